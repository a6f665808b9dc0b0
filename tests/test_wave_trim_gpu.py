"""The wave kernel's EVSE extent (P = Ghat r0 over the k-steps that hold an EVSE of the site; acn_qp_rank.hpp, DESIGN.md
section 3.1) may not change a bit.

  * against the PARENT commit: tests/golden/wave_trim.npz holds the cases of tests/wave_trim_cases.py as the parent's
    library solved them on the MI355X (tools/make_golden_wave_trim.py) -- array_equal of x, status, iters, pri_res,
    dua_res, obj;
  * against the full extent: ACNQP_WAVE_FULL_EVSE=1 is read once per process, so the cases are solved in two child
    processes -- all of them in each -- and compared here; what acnqp_debug_wave_evse_extent reports is asserted for
    every case, so that no case can pass by running the same extent twice."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import wave_trim_cases as TC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_trim.npz")
N_EVSE = {"c54_h12": 54, "jpl52_h24": 52, "c54_h24": 54, "s36_h12": 36, "syn56": 56, "syn57": 57, "warm": 54}
EXTENT = {"c54_h12": 14, "jpl52_h24": 14, "c54_h24": 14, "s36_h12": 14, "syn56": 14, "syn57": 16, "warm": 14}   # (N <= 56: 14 k-steps)


@functools.lru_cache(maxsize=None)
def _runs():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, env in (("site", {}), ("full", {"ACNQP_WAVE_FULL_EVSE": "1"})):
            f = os.path.join(tmp, tag + ".npz")
            e = {k: v for k, v in os.environ.items() if k not in ("ACNQP_WAVE_FULL_RANK", "ACNQP_WAVE_FULL_EVSE", "ACNQP_NO_WAVE", "ACNQP_NO_WAVE2", "ACNQP_WAVE_MIN_BATCH")}
            subprocess.run([sys.executable, TC.__file__, f], check=True, env=dict(e, **env), timeout=600)
            with np.load(f) as z:
                out[tag] = {k: z[k] for k in z.files}
    return out


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _case(run, name):
    return {k.split(":", 1)[1]: v for k, v in run.items() if k.startswith(name + ":")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", TC.CASES)
def test_this_build_gives_the_bits_of_the_parent(name):
    got, want = _case(_runs()["site"], name), _case(_golden(), name)
    assert str(got["family"]) == TC.FAMILY[name]
    assert (int(got["n_evse"]), int(got["evse_ksteps"]), int(got["extent"])) == (N_EVSE[name], -(-N_EVSE[name] // 4), EXTENT[name])
    assert sorted(want) == sorted(TC.KEYS)
    for key in TC.KEYS:
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (name, key, np.abs(got[key].astype(float) - want[key].astype(float)).max())
    # what the case is there for: the ring wraps (5 slots, one event per 5 iterations: every slot written twice by 60)
    assert want["iters"].max() >= 60, (name, want["iters"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", TC.CASES)
def test_site_extent_gives_the_bits_of_all_sixteen_ksteps(name):
    site, full = _case(_runs()["site"], name), _case(_runs()["full"], name)
    assert str(full["family"]) == TC.FAMILY[name]
    assert int(site["extent"]) == EXTENT[name] and int(full["extent"]) == 16, (name, site["extent"], full["extent"])
    assert (int(full["n_evse"]), int(full["evse_ksteps"])) == (N_EVSE[name], -(-N_EVSE[name] // 4))
    for key in TC.KEYS:
        assert np.array_equal(site[key], full[key]), (name, key, np.abs(site[key].astype(float) - full[key].astype(float)).max())
