"""Where the wave kernel's vector work stands relative to its matrix chains (the window masks decoded only where they are
read; acn_qp_wave.hpp, DESIGN.md section 3.1 "overlap") may not change a bit: tests/golden/wave_overlap.npz holds the
cases of tests/wave_overlap_cases.py as the PARENT commit's library solved them on the MI355X (tools/make_golden_wave_overlap.py) -- array_equal of x, status, iters, pri_res, dua_res, obj,
and of y where the case asks for it.  All cases are solved once, in one child process, and shared."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import wave_overlap_cases as OC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_overlap.npz")


@functools.lru_cache(maxsize=None)
def _run():
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "this.npz")
        env = {k: v for k, v in os.environ.items() if not k.startswith("ACNQP_")}
        subprocess.run([sys.executable, OC.__file__, f], check=True, env=env, timeout=600)
        with np.load(f) as z:
            return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _case(run, name):
    return {k.split(":", 1)[1]: v for k, v in run.items() if k.startswith(name + ":")}


def test_the_cases_hold_what_they_were_picked_for():
    """on the CPU twin: a problem of >= 60 iterations and one that adapts rho; the equality case's start point clips every period"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_golden_wave_overlap

    make_golden_wave_overlap.check_twin()
    assert all(len(pick) <= 8 for _, _, pick in OC.PICK.values()) and sorted(OC.FAMILY) == sorted(OC.CASES)
    prox = [n for n in OC.CASES if n.startswith(("dc", "flat"))]
    assert {OC.FAMILY[n] for n in prox} == {"wave1", "wave2", "wave3", "wave4"}   # every variant runs a PROX instantiation


@pytest.mark.gpu
@pytest.mark.parametrize("name", OC.CASES)
def test_this_build_gives_the_bits_of_the_parent(name):
    got, want = _case(_run(), name), _case(_golden(), name)
    keys = OC.KEYS + (("y",) if name in OC.WITH_Y else ())
    assert str(got["family"]) == OC.FAMILY[name]
    assert sorted(want) == sorted(keys)
    assert len(want["iters"]) <= 8
    for key in keys:
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (name, key, np.abs(got[key].astype(float) - want[key].astype(float)).max())
    # what the cases are there for
    if name in OC.LONG_AND_ADAPTING:
        assert want["iters"].max() >= 60, (name, want["iters"])
    if name == "hand_over":   # (a handed-over problem ends with the polish's status or resumes: it ran the hand-over's y_out)
        assert np.any(want["y"] != 0.0)
