"""The EVSE extent of the wave kernel's P = Ghat r0 (wave_evse_extent, adacharge_amd/csrc/acn_qp_rank.hpp), compiled for
the host as tests/test_wave_rank.py compiles the rank analysis, and pinned without a GPU.  The expected values are
written out here, never computed by the header."""
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adacharge_amd", "csrc")

SHIM = r"""
#include "acn_qp_rank.hpp"
extern "C" int evse_extent(int n, int full_evse) { return acnqp::wave_evse_extent(n, full_evse != 0); }
"""


@functools.lru_cache(maxsize=None)
def _lib():
    tmp = tempfile.mkdtemp(prefix="acnqp_trim_")
    src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.run([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    shutil.rmtree(tmp)   # (the mapping stays; nothing built is left behind)
    lib.evse_extent.restype, lib.evse_extent.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int]
    return lib


def test_extent_is_fourteen_ksteps_up_to_56_evses_and_sixteen_beyond():
    want = {1: 14, 30: 14, 36: 14, 52: 14, 53: 14, 54: 14, 55: 14, 56: 14, 57: 16, 60: 16, 63: 16, 64: 16}
    assert {n: _lib().evse_extent(n, 0) for n in want} == want


def test_the_extent_always_holds_every_evse_of_the_site():
    for n in range(1, 65):
        assert 4 * _lib().evse_extent(n, 0) >= n, n


def test_the_switch_forces_all_sixteen():
    assert [_lib().evse_extent(n, 1) for n in (1, 36, 54, 56, 57, 64)] == [16] * 6
