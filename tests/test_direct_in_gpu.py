"""The direct path for lb / ub / q: with PINNED lb, ub and q the wave kernel (one wave per problem)
loads the inputs of the leading chunk of a call of several chunks straight from the caller's arrays and completes the chunk's device copy
itself; the chunk loop queues no copy of the three.  Every case of tests/direct_in_cases.py is solved in this process with
the path on and, once for all cases, in a child process with ACNQP_NO_DIRECT_IN=1 (read once per process): x, status,
iters, pri_res, dua_res and obj must be equal bit for bit, and acnqp_debug_direct_in must report the number of problems
the case means to load directly -- 0 in the child."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import direct_in_cases as IC

SWITCHES = ("ACNQP_NO_DIRECT_IN", "ACNQP_NO_DIRECT_X", "ACNQP_PLAN", "ACNQP_CHUNK", "ACNQP_NO_RAMP", "ACNQP_NO_STAGING", "ACNQP_NO_WAVE",
            "ACNQP_WAVE_MIN_BATCH", "ACNQP_NO_POLISH", "ACNQP_NO_ORDER", "ACNQP_NO_QUEUE")


@pytest.fixture(scope="module")
def copied(tmp_path_factory):
    """every case through the copy path, solved once"""
    f = str(tmp_path_factory.mktemp("direct_in") / "off.npz")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    subprocess.run([sys.executable, IC.__file__, f], check=True, env=dict(env, ACNQP_NO_DIRECT_IN="1"), timeout=600)
    with np.load(f) as z:
        return {k: z[k] for k in z.files}


def _same(name, copied, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    _, meant = IC.build(name)
    got, direct, polish = IC.solve(name)
    print(f"[direct in] {name}: {direct} problems loaded directly (meant: {meant}), the child {int(copied[f'{name}:direct'])}")
    assert direct == meant, name
    assert int(copied[f"{name}:direct"]) == 0, name
    for k in IC.KEYS:
        ref = copied[f"{name}:{k}"]
        assert got[k].shape == ref.shape and np.array_equal(got[k], ref), (name, k)
    assert not (got["status"] == 0).any(), name
    return got, polish


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n64_t12", "n54_t12", "n5_t7", "n64_t1"])
def test_flat_loop_tails(name, copied, monkeypatch):
    _same(name, copied, monkeypatch)


@pytest.mark.gpu
def test_horizon_12_behind_horizon_7_on_one_handle(copied, monkeypatch):
    _same("t12_after_t7", copied, monkeypatch)


@pytest.mark.gpu
def test_handed_over_problems_read_a_complete_device_copy(copied, monkeypatch):
    got, polish = _same("hand_over", copied, monkeypatch)
    print("handed over", polish["attempted"], "polished", polish["solved"])
    assert polish["attempted"] >= 8 and polish["solved"] >= 1
    assert not (got["status"] == 6).any()


@pytest.mark.gpu
def test_early_hand_over_polish_and_resume_launch(copied, monkeypatch):
    got, polish = _same("hand_over_early", copied, monkeypatch)
    print("handed over", polish["attempted"], "polished", polish["solved"], "passed on to the resume launch", polish["attempted"] - polish["solved"])
    assert polish["attempted"] >= 8
    assert not (got["status"] == 6).any()


@pytest.mark.gpu
def test_retry_pass_reads_a_complete_device_copy(copied, monkeypatch):
    got, _ = _same("retry", copied, monkeypatch)
    assert (got["iters"] > 200).any()   # (more than pass 0 may take: a retry pass ran)


@pytest.mark.gpu
def test_empty_set_and_infeasible_verdicts(copied, monkeypatch):
    got, _ = _same("verdicts", copied, monkeypatch)
    assert got["status"].ravel().tolist() == [1, 4, 1, 3, 1]   # (the empty-set and the infeasible problem are in the leading chunk)


@pytest.mark.gpu
def test_pinned_and_pageable_batches_in_one_call(copied, monkeypatch):
    _same("mixed", copied, monkeypatch)


@pytest.mark.gpu
def test_a_batch_whose_q_alone_is_pageable_keeps_its_copies(copied, monkeypatch):
    _same("q_pageable", copied, monkeypatch)


@pytest.mark.gpu
def test_only_the_leading_chunk_loads_directly(copied, monkeypatch):
    _same("two_chunks", copied, monkeypatch)


@pytest.mark.gpu
def test_warm_start_with_multipliers(copied, monkeypatch):
    _same("warm", copied, monkeypatch)


@pytest.mark.gpu
def test_launch_order_by_session_count_gives_the_same_bits(copied, monkeypatch):
    _same("launch_order", copied, monkeypatch)


@pytest.mark.gpu
def test_a_call_of_one_chunk_keeps_its_copies(copied, monkeypatch):
    _same("one_chunk", copied, monkeypatch)
