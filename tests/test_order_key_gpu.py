"""The launch-order key on the device (order_keys_kernel, adacharge_amd/csrc/acn_qp_pipeline.hpp; read through
SiteHandle.order_keys) against its numpy definition (tests/order_key_spec.py), equal key for key, on every shape the
kernel treats differently; and one launch of 1,024 problems sorted by either key (ACNQP_ORDER_KEY), equal bit for bit.

Every case first asserts, on the spec side, that no cell's load / limit lies within 1e-6 of 1: the device sums a row's
load in another order than numpy, and a difference of rounding can then never decide a key.  No problem is excluded.

Run as a script it solves the launch case under the environment it was started with and saves the results."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import order_key_spec as spec  # noqa: E402

CHILD_TIMEOUT = 120   # seconds per child process of the launch case


def _build(infra, lists, cone="SOC", es=1e-12, peak_limits=None):
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge
    from adacharge_amd.acn import Interface
    from adacharge_amd.builder import build_batch

    iface = Interface({"infrastructure_info": infra, "period": 5})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, es)]
    return build_batch(lists, infra, iface, obj, cone, peak_limits=peak_limits)


def _general(infra, T, B, seed, **kw):
    from adacharge_amd import sites

    return [sites.random_sessions_general(infra, T, np.random.default_rng(c), **kw) for c in np.random.SeedSequence(seed).spawn(B)]


def case_caltech_soc():
    from adacharge_amd import sites

    infra = sites.caltech54()
    return _build(infra, sites.snapshot_batch(infra, 12, 64, seed=9101))


def case_caltech_linear():
    from adacharge_amd import sites

    infra = sites.caltech54()
    return _build(infra, sites.snapshot_batch(infra, 12, 64, seed=9102), cone="LINEAR")


def case_horizon7_minimum_rates():
    """lb > 0 over a prefix of the windows, delayed arrivals, problem b's sessions drawn for a horizon of 3 + b % 5 periods"""
    from adacharge_amd import sites

    infra = sites.caltech54()
    lists = [sites.random_sessions_general(infra, 3 + b % 5, np.random.default_rng(c), min_rates=True)
             for b, c in enumerate(np.random.SeedSequence(9103).spawn(48))]
    return _build(infra, lists)


def case_site3_two_row_tiles():
    """configs[3] site 3: 36 EVSEs, 9 disc pairs = 18 site rows, which straddle the solver's 16-row tile; demand scenarios"""
    from adacharge_amd import sites
    from adacharge_amd.builder import scenario_batch

    infra = sites.eight_sites()[3]
    rng = np.random.default_rng(9104)
    base = _build(infra, [sites.random_sessions(infra, 12, rng)], es=1e-3)
    return scenario_batch(base, rng.lognormal(0.0, 0.25, size=(48, base.K, base.N)))


def case_two_session_slots():
    from adacharge_amd import sites

    infra = sites.caltech54()
    return _build(infra, _general(infra, 12, 48, 9105, two_per_evse=True))


def case_peak_row():
    """a peak limit per period: none (+inf) in every third period, else 150 ... 600 A"""
    from adacharge_amd import sites

    infra = sites.caltech54()
    rng = np.random.default_rng(9106)
    peaks = [np.where(np.arange(12) % 3 == b % 3, np.inf, rng.uniform(150.0, 600.0, size=12)) for b in range(48)]
    return _build(infra, sites.snapshot_batch(infra, 12, 48, seed=9106), peak_limits=peaks)


def case_largest_inside_budget():
    """54 x 144: 62,208 bytes of schedule, two problems per workgroup"""
    from adacharge_amd import sites

    infra = sites.caltech54()
    return _build(infra, sites.snapshot_batch(infra, 144, 32, seed=9107, demand_range=(5.0, 60.0)))


def case_beyond_budget():
    """54 x 152: 65,664 bytes of schedule, more than the kernel's 64 KB: the session count is the key"""
    from adacharge_amd import sites

    infra = sites.caltech54()
    return _build(infra, sites.snapshot_batch(infra, 152, 32, seed=9108, demand_range=(5.0, 60.0)))


def case_four_wave_route():
    """jpl52 x 24: two row tiles x horizon 24, the wave kernel's four-wave route, which keeps the session count as its key"""
    from adacharge_amd import sites

    infra = sites.jpl52()
    return _build(infra, sites.snapshot_batch(infra, 24, 32, seed=9110), es=1e-3)


# name -> (builder, the kernel's key is the congestion key)
CASES = {
    "caltech54 x 12 SOC": (case_caltech_soc, True),
    "caltech54 x 12 LINEAR": (case_caltech_linear, True),
    "horizon 7, minimum rates, mixed horizons": (case_horizon7_minimum_rates, True),
    "36 EVSEs, 18 site rows": (case_site3_two_row_tiles, True),
    "two session slots": (case_two_session_slots, True),
    "peak row": (case_peak_row, True),
    "54 x 144, largest inside the LDS budget": (case_largest_inside_budget, True),
    "54 x 152, beyond the LDS budget": (case_beyond_budget, False),
    "jpl52 x 24, the four-wave route": (case_four_wave_route, False),
}


def expected(name):
    """(batch, keys the device must report); asserts what the case is there for, and the rounding margin"""
    build, congestion = CASES[name]
    batch = build()
    assert 32 <= batch.B <= 64
    ratios, C, keys = spec.describe(batch)
    assert spec.margin(ratios) > 1e-6, f"{name}: a cell ratio within 1e-6 of 1"
    assert (C > 0).any() and len(np.unique(keys)) > 4, f"{name}: the case does not exercise the key"
    if name.startswith("horizon 7"):
        assert (batch.lb > 0).any() and len(np.unique(batch.T)) > 2 and batch.Tm == 7
    if name.startswith("36 EVSEs"):
        assert batch.N == 36 and batch.site.Mg == 18
    if name.startswith("two session"):
        assert batch.K == 2 and (np.asarray(batch.s_len)[:, 1] > 0).any()
    if name.startswith("peak"):
        assert batch.site.has_peak and np.isinf(batch.peak).any() and (ratios[:, -1] > spec.OVERLOAD).any()
    if name.startswith("54 x 144"):
        assert (batch.N, batch.Tm) == (54, 144) and batch.N * batch.Tm * 8 <= 65536
    if name.startswith("54 x 152"):
        assert batch.N * batch.Tm * 8 > 65536
    if not congestion:
        keys = spec.session_keys(batch)
        assert len(np.unique(keys)) > 4
    return batch, keys


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_keys_equal_the_spec(hip_library, name):
    import torch

    from adacharge_amd.backend import DeviceBatch, SiteHandle

    batch, keys = expected(name)
    h = SiteHandle(batch.site, 0)
    try:
        db = DeviceBatch(batch, torch.device("cuda", 0))
        torch.cuda.synchronize()
        got = h.order_keys(db)
        assert (h.route(batch.Tm, batch.K, batch.B)[0] == "wave4") == name.startswith("jpl52")
    finally:
        h.close()
    assert got.dtype == np.int32 and np.array_equal(got, keys)


# ---- one launch of 1,024 problems under either key ---------------------------------------------------------------------
FIELDS = ("x", "status", "iters", "pri_res", "dua_res", "obj")


def solve_launch():
    """the headline shape, 1,024 problems in ONE launch (acnqp_solve_batch_device: the launch order engages)"""
    import torch

    from adacharge_amd import sites
    from adacharge_amd.backend import DeviceBatch, SiteHandle, default_options

    infra = sites.caltech54()
    batch = _build(infra, sites.snapshot_batch(infra, 12, 1024, seed=9109))
    h = SiteHandle(batch.site, 0)
    db = DeviceBatch(batch, torch.device("cuda", 0))
    h.solve_device(db, default_options(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = {k: getattr(db, k).cpu().numpy() for k in FIELDS}
    out.update(ordered=np.array(h.ordered_launches()), keys=h.order_keys(db))
    h.close()
    return out, batch


@pytest.mark.gpu
def test_either_key_gives_the_same_results(hip_library, tmp_path):
    runs = {}
    for tag, value in (("overload", None), ("sessions", "sessions")):
        env = {k: v for k, v in os.environ.items() if k not in ("ACNQP_ORDER_KEY", "ACNQP_NO_ORDER", "ACNQP_NO_QUEUE")}
        if value:
            env["ACNQP_ORDER_KEY"] = value
        path = str(tmp_path / f"{tag}.npz")
        subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, timeout=CHILD_TIMEOUT)
        runs[tag] = np.load(path)
    a, b = runs["overload"], runs["sessions"]
    assert int(a["ordered"]) == 1 and int(b["ordered"]) == 1
    assert np.array_equal(b["keys"], b["session_keys"]) and not np.array_equal(a["keys"], b["keys"])   # the switch switched
    for k in FIELDS:
        assert np.array_equal(a[k], b[k]), k


if __name__ == "__main__":
    out, batch = solve_launch()
    np.savez(sys.argv[1], session_keys=spec.session_keys(batch), **out)
