"""The chunk planner (adacharge_amd/csrc/acn_qp_pipeline.hpp) for a call whose schedules the kernel stores into the
caller's arrays itself (PlanEnv::direct): no small last chunk -- the small chunks in front, the
largest last (u, 2u, 2u, then chunks of 3u).  Compiled for the host like tests/test_route_table.py; the expected sizes are written out here, not
computed by the header.  Without `direct` the planner answers as tests/test_route_table.py::test_planner pins it."""
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adacharge_amd", "csrc")
INC = os.path.join(ROOT, "include")

SHIM = r"""
#include "acn_qp_route.hpp"
#include "acn_qp_pipeline.hpp"
using namespace acnqp;
extern "C" {
// the chunk sizes of a uniform wave call, as the chunk loop realises the planner's caps
int chunks(long long total, long long want, long long by_mem, const char* plan, int direct, long long* out, int n) {
  PlanEnv env; env.plan = plan; env.direct = direct != 0;
  const std::vector<long long> caps = plan_chunk_caps(total, want, by_mem, true, true, env);
  int c = 0;
  for (long long lo = 0; lo < total && c < n; ++c) { out[c] = std::min(total - lo, chunk_cap(caps, c)); lo += out[c]; }
  return c;
}
// which routes can store x into a host array: by shape alone
int direct_x(int N, int M, int T, int K, int batch) { return route_for(site_shape(N, M, 0, 0, 0, 0), T, K, batch, RouteSwitches()).direct_x(); }
}
"""


@functools.lru_cache(maxsize=None)
def _lib():
    tmp = tempfile.mkdtemp(prefix="acnqp_direct_plan_")
    src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.run([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-I" + INC, src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    shutil.rmtree(tmp)
    LL, I = ctypes.c_longlong, ctypes.c_int
    lib.chunks.restype, lib.chunks.argtypes = I, [LL, LL, LL, ctypes.c_char_p, I, ctypes.POINTER(LL), I]
    lib.direct_x.restype, lib.direct_x.argtypes = I, [I] * 5
    return lib


def _chunks(total, want=8192, by_mem=1 << 40, plan=None, direct=True):
    out = (ctypes.c_longlong * 64)()
    n = _lib().chunks(total, want, by_mem, None if plan is None else plan.encode(), int(direct), out, 64)
    return [int(out[i]) for i in range(n)]


def test_direct_plans_as_literals():
    """u, 2u, 2u in front, then m chunks of 3u: u = ceil(total / (5 + 3m)), the smallest m with 3u <= cap"""
    assert _chunks(2047) == [2047]                                   # under 2,048 problems: one chunk
    assert _chunks(4096) == [512, 1024, 1024, 1536]
    assert _chunks(16384) == [2048, 4096, 4096, 6144]                # the headline call
    assert _chunks(20000) == [2500, 5000, 5000, 7500]
    assert _chunks(2048) == [256, 512, 512, 768]
    assert _chunks(20000, want=2048) == [625, 1250, 1250] + [1875] * 9     # m = 9: u = 625
    assert _chunks(6145, want=2048) == [558, 1116, 1117, 1677, 1677]       # m = 2: u = 559, a front of 2,791
    assert _chunks(16384, by_mem=5000) == [1488, 2977, 2979, 4470, 4470]   # the cap by memory: 4,608; u = 1,490, a front of 7,444


@pytest.mark.parametrize("total", [2047, 2048, 4096, 6145, 8191, 8192, 8193, 16384, 16385, 20000, 24575, 24576, 24577, 100000])
@pytest.mark.parametrize("want,by_mem", [(8192, 1 << 40), (8192, 5000), (2048, 1 << 40)])
def test_direct_plan_properties(total, want, by_mem):
    cap = min(want, by_mem)
    cap -= cap % 512
    got = _chunks(total, want, by_mem)
    assert sum(got) == total and min(got) >= 1
    if total < 2048:
        assert got == [total]
        return
    assert max(got) <= cap, got                 # no chunk above the cap
    assert got[-1] == max(got), got             # the last chunk is the largest
    assert got[0] <= got[-1] // 2 or len(got) == 1, got


def test_an_explicit_plan_still_wins():
    assert _chunks(96, plan="8,16,0,24") == [8, 16, 1, 24, 47]
    assert _chunks(16384, plan="2048,4096,4096") == [2048, 4096, 4096, 6144]


def test_without_direct_the_planner_answers_as_before():
    assert _chunks(16384, direct=False) == [2048, 4096, 8192, 2048]
    assert _chunks(2047, direct=False) == [2047]
    assert _chunks(4096, direct=False) == [1024, 2048, 1024]
    assert _chunks(20000, direct=False) == [1664, 3328, 6656, 6656, 1696]
    assert _chunks(96, plan="8,16,8,24,8", direct=False) == [8, 16, 8, 24, 8, 32]


def test_the_capability_is_decided_by_shape_alone():
    d = _lib().direct_x
    assert [d(54, 10, 12, 1, b) for b in (1, 256, 16384)] == [1, 1, 1]     # wave1, whatever the batch
    assert d(64, 10, 12, 1, 1) == 1 and d(1, 1, 1, 1, 1) == 1
    assert d(54, 10, 13, 1, 1) == 0 and d(54, 20, 12, 1, 1) == 0           # wave2, wave3: more than one wave per problem
    assert d(54, 10, 12, 2, 1) == 0 and d(65, 10, 12, 1, 1) == 0           # tiled, large-site
