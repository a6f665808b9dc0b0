"""The rank analysis behind the wave kernel's eigen extent (adacharge_amd/csrc/acn_qp_rank.hpp), compiled for the host
(g++, as tests/test_route_table.py compiles the routing table) and pinned without a GPU.  The expected values are
written out here, never computed by the header."""
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adacharge_amd", "csrc")

SHIM = r"""
#include "acn_qp_rank.hpp"
using namespace acnqp;
extern "C" {
// out: rank, eig_ksteps; perm[n]
void rank_of(const double* lam, int n, int* out, int* perm) {
  const EigRank e = eig_rank(std::vector<double>(lam, lam + n));
  out[0] = e.rank; out[1] = e.eig_ksteps; out[2] = (int)e.perm.size();
  for (int k = 0; k < n && k < (int)e.perm.size(); ++k) perm[k] = e.perm[k];
}
int extent(int eig_ksteps, int full_rank) { return wave_eig_extent(eig_ksteps, full_rank != 0); }
}
"""


@functools.lru_cache(maxsize=None)
def _lib():
    tmp = tempfile.mkdtemp(prefix="acnqp_rank_")
    src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.run([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    shutil.rmtree(tmp)   # (the mapping stays; nothing built is left behind)
    I = ctypes.c_int
    lib.rank_of.restype, lib.rank_of.argtypes = None, [ctypes.POINTER(ctypes.c_double), I, ctypes.POINTER(I), ctypes.POINTER(I)]
    lib.extent.restype, lib.extent.argtypes = I, [I, I]
    return lib


def _rank(lam):
    lam = np.asarray(lam, dtype=np.float64)
    out, perm = (ctypes.c_int * 3)(), (ctypes.c_int * max(1, len(lam)))()
    _lib().rank_of(lam.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(lam), out, perm)
    assert out[2] == len(lam)
    return int(out[0]), int(out[1]), [int(perm[k]) for k in range(len(lam))]


def _lam(n, live):
    lam = np.zeros(n)
    lam[list(live)] = 1.0 + np.arange(len(live))
    return lam


def test_perm_is_a_stable_partition_live_first():
    # the headline site's pattern: live eigen-rows 1 2 4 5 7 8 9 of 16
    rank, ks, perm = _rank(_lam(16, (1, 2, 4, 5, 7, 8, 9)))
    assert (rank, ks) == (7, 2)
    assert perm == [1, 2, 4, 5, 7, 8, 9, 0, 3, 6, 10, 11, 12, 13, 14, 15]
    # already compact, all null, all live: the identity
    for live in (range(5), (), range(16)):
        assert _rank(_lam(16, live))[2] == list(range(16))
    # live eigenpairs in the second tile of a two-tile site move to the front, order kept on both sides
    rank, ks, perm = _rank(_lam(32, (3, 17, 18, 30)))
    assert (rank, ks) == (4, 1) and perm[:4] == [3, 17, 18, 30] and perm[4:] == [k for k in range(32) if k not in (3, 17, 18, 30)]
    # every permutation is one, whatever the pattern; a tiny but non-zero eigenvalue is live (the zeroing is build_site_dev's)
    rng = np.random.default_rng(3)
    for _ in range(50):
        n = int(rng.choice([16, 32, 48]))
        lam = np.where(rng.random(n) < 0.5, 0.0, rng.uniform(1e-300, 5.0, n))
        rank, ks, perm = _rank(lam)
        live = [k for k in range(n) if lam[k] != 0.0]
        assert sorted(perm) == list(range(n)) and perm[:rank] == live and perm[rank:] == [k for k in range(n) if lam[k] == 0.0]
        assert rank == len(live) and ks == -(-rank // 4)


def test_eig_ksteps_at_the_four_row_boundaries():
    want = {0: 0, 1: 1, 4: 1, 5: 2, 8: 2, 9: 3, 12: 3, 13: 4, 16: 4}
    for rank, ks in want.items():
        # the live rows scattered from the back: the count alone decides
        assert _rank(_lam(16, range(16 - rank, 16)))[:2] == (rank, ks), rank
    assert _rank(_lam(32, range(0, 32, 2)))[:2] == (16, 4)
    assert _rank(_lam(32, range(15, 32)))[:2] == (17, 5)


def test_extent_is_the_smallest_specialised_one_that_holds_the_rank_or_the_full_one():
    ext = _lib().extent
    # 0 = the full extent: every k-step on the shared eigenbasis (the kernel as it was)
    assert [ext(ks, 0) for ks in range(0, 9)] == [2, 2, 2, 3, 0, 0, 0, 0, 0]
    # a rank above one eigen tile on a two-tile site (17 ... 32 live rows: 5 ... 8 k-steps) asks for the full extent
    assert ext(_rank(_lam(32, range(15, 32)))[1], 0) == 0
    # ACNQP_WAVE_FULL_RANK=1: the full extent whatever the rank
    assert [ext(ks, 1) for ks in range(0, 9)] == [0] * 9
