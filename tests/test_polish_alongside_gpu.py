"""The polish launch that runs alongside the solver launch changes WHEN a handed-over problem is
polished, never what comes out: every case of tests/polish_alongside_cases.py is solved in child processes -- the switches
are read once per process -- with the launch alongside (the default), without it (ACNQP_NO_POLISH_ALONGSIDE=1) and, the first
case, with workgroups alongside that give up at once (ACNQP_POLISH_ALONGSIDE_SPINS=0), and compared here with array_equal."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import polish_alongside_cases as PC

SWITCHES = ("ACNQP_NO_POLISH_ALONGSIDE", "ACNQP_POLISH_ALONGSIDE_SPINS", "ACNQP_POLISH_ALONGSIDE_GRID", "ACNQP_NO_POLISH", "ACNQP_NO_WAVE",
            "ACNQP_NO_WAVE2", "ACNQP_WAVE_MIN_BATCH", "ACNQP_NO_QUEUE", "ACNQP_EARLY_HANDOVER", "ACNQP_CHUNK", "ACNQP_PLAN")
STATUS_UNSET = 0


@functools.lru_cache(maxsize=None)
def _runs():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, env, names in (("on", {}, ()), ("off", {"ACNQP_NO_POLISH_ALONGSIDE": "1"}, ()), ("bail", {"ACNQP_POLISH_ALONGSIDE_SPINS": "0"}, ("lone_h12",))):
            f = os.path.join(tmp, tag + ".npz")
            e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
            subprocess.run([sys.executable, PC.__file__, f, *names], check=True, env=dict(e, **env), timeout=300)
            with np.load(f) as z:
                out[tag] = {k: z[k] for k in z.files}
    return out


def _case(tag, name):
    return {k.split(":", 1)[1]: v for k, v in _runs()[tag].items() if k.startswith(name + ":")}


def _same_results(a, b, name):
    for key in PC.KEYS:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), (name, key, np.abs(a[key].astype(float) - b[key].astype(float)).max())


def _handed_over(case, name):
    """At least 8 problems of the case went to the polish, and the statuses hold nothing internal or unset."""
    print(name, "handed over", int(case["attempted"]), "polished", int(case["solved"]), "taken alongside", int(case["alongside"]))
    assert int(case["attempted"]) >= 8, (name, case["attempted"])
    assert not np.any(case["status"] == STATUS_UNSET) and not np.any(case["status"] == 6), name


@pytest.mark.gpu
def test_lone_h12():
    on, off = _case("on", "lone_h12"), _case("off", "lone_h12")
    assert str(on["family"]) == "wave1"
    _handed_over(on, "lone_h12")
    _same_results(on, off, "lone_h12")
    assert int(on["alongside"]) > 0 and int(off["alongside"]) == 0, (on["alongside"], off["alongside"])


@pytest.mark.gpu
def test_one_per_wave():
    on, off = _case("on", "one_per_wave"), _case("off", "one_per_wave")
    _handed_over(on, "one_per_wave")
    _same_results(on, off, "one_per_wave")
    assert int(off["alongside"]) == 0


@pytest.mark.gpu
def test_pipelined_last_chunk():
    on, off = _case("on", "pipelined_last_chunk"), _case("off", "pipelined_last_chunk")
    _handed_over(on, "pipelined_last_chunk")
    _same_results(on, off, "pipelined_last_chunk")
    assert not np.any(on["status"] == STATUS_UNSET)
    assert int(off["alongside"]) == 0


@pytest.mark.gpu
def test_bail_out():
    bail, off = _case("bail", "lone_h12"), _case("off", "lone_h12")
    _handed_over(bail, "bail_out")
    _same_results(bail, off, "bail_out")
    # a bound of 0 polls: every workgroup alongside leaves before its first look at the list (acn_qp_polclaim.hpp), so the
    # launches alongside take NOTHING and the serial launch polishes everything -- while the same case with the default
    # bound takes problems alongside (a switch that was not honoured would fail here)
    assert int(bail["alongside"]) == 0, bail["alongside"]
    assert int(_case("on", "lone_h12")["alongside"]) > 0
    assert (int(bail["attempted"]), int(bail["solved"])) == (int(off["attempted"]), int(off["solved"]))


@pytest.mark.gpu
def test_h24_two_waves():
    on, off = _case("on", "h24_two_waves"), _case("off", "h24_two_waves")
    assert str(on["family"]) == "wave2"
    _handed_over(on, "h24_two_waves")
    _same_results(on, off, "h24_two_waves")
    assert int(off["alongside"]) == 0


@pytest.mark.gpu
def test_pol_stats():
    on, off = _case("on", "lone_h12"), _case("off", "lone_h12")
    assert (int(on["attempted"]), int(on["solved"])) == (int(off["attempted"]), int(off["solved"])), (on["attempted"], on["solved"], off["attempted"], off["solved"])
