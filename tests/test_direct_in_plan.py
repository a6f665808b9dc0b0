"""The chunk planner (adacharge_amd/csrc/acn_qp_pipeline.hpp) under PlanEnv::direct_in -- the kernel loads the leading chunk's
lb / ub / q from the caller's arrays itself.  With the flag off every total that
tests/test_direct_plan.py pins gives the plan written out there (restated here as literals); with it on the plan obeys the
same properties: the sizes sum to the call, none is above the cap.  Also: which routes can load from the host, by shape
alone, and the one row of the chunk table that carries the sources.  Compiled for the host like tests/test_direct_plan.py."""
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
int chunks(long long total, long long want, long long by_mem, const char* plan, int direct, int direct_in, long long* out, int n) {
  PlanEnv env; env.plan = plan; env.direct = direct != 0; env.direct_in = direct_in != 0;
  const std::vector<long long> caps = plan_chunk_caps(total, want, by_mem, true, true, env);
  int c = 0;
  for (long long lo = 0; lo < total && c < n; ++c) { out[c] = std::min(total - lo, chunk_cap(caps, c)); lo += out[c]; }
  return c;
}
int direct_in(int N, int M, int T, int K, int batch) { return route_for(site_shape(N, M, 0, 0, 0, 0), T, K, batch, RouteSwitches()).direct_in(); }
// the row of host addresses of a chunk of cn problems: o = {start of the row, its bytes, the four tables' starts}
void host_row(long long cn, int direct, int direct_in, long long* o) {
  ChunkShape s{54, 12, 1, 5, false, false, false, false, false, direct != 0};
  s.direct_in = direct_in != 0;
  const ChunkLayout L((size_t)cn, s);
  o[0] = (long long)L.in[kXh]; o[1] = (long long)(L.in[kXh + 1] - L.in[kXh]);
  for (int k = 0; k < 4; ++k) o[2 + k] = (long long)L.host_table((HostTable)k);
  o[6] = (long long)(L.mirror_in() + L.mirror_in_bytes());
}
}
"""


@functools.lru_cache(maxsize=None)
def _lib():
    tmp = tempfile.mkdtemp(prefix="acnqp_direct_in_plan_")
    src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.run([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-I" + INC, src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    shutil.rmtree(tmp)
    LL, I = ctypes.c_longlong, ctypes.c_int
    lib.chunks.restype, lib.chunks.argtypes = I, [LL, LL, LL, ctypes.c_char_p, I, I, ctypes.POINTER(LL), I]
    lib.direct_in.restype, lib.direct_in.argtypes = I, [I] * 5
    lib.host_row.restype, lib.host_row.argtypes = None, [LL, I, I, ctypes.POINTER(LL)]
    return lib


def _chunks(total, want=8192, by_mem=1 << 40, plan=None, direct=True, direct_in=False):
    out = (ctypes.c_longlong * 64)()
    n = _lib().chunks(total, want, by_mem, None if plan is None else plan.encode(), int(direct), int(direct_in), out, 64)
    return [int(out[i]) for i in range(n)]


def test_with_the_flag_off_every_pinned_plan_is_what_it_was():
    assert _chunks(2047) == [2047]
    assert _chunks(4096) == [512, 1024, 1024, 1536]
    assert _chunks(16384) == [2048, 4096, 4096, 6144]
    assert _chunks(20000) == [2500, 5000, 5000, 7500]
    assert _chunks(2048) == [256, 512, 512, 768]
    assert _chunks(20000, want=2048) == [625, 1250, 1250] + [1875] * 9
    assert _chunks(6145, want=2048) == [558, 1116, 1117, 1677, 1677]
    assert _chunks(16384, by_mem=5000) == [1488, 2977, 2979, 4470, 4470]
    assert _chunks(96, plan="8,16,0,24") == [8, 16, 1, 24, 47]
    assert _chunks(16384, plan="2048,4096,4096") == [2048, 4096, 4096, 6144]
    assert _chunks(16384, direct=False) == [2048, 4096, 8192, 2048]
    assert _chunks(2047, direct=False) == [2047]
    assert _chunks(4096, direct=False) == [1024, 2048, 1024]
    assert _chunks(20000, direct=False) == [1664, 3328, 6656, 6656, 1696]
    assert _chunks(96, plan="8,16,8,24,8", direct=False) == [8, 16, 8, 24, 8, 32]


@pytest.mark.parametrize("total", [1, 2047, 2048, 4096, 6145, 8191, 8192, 8193, 16384, 16385, 20000, 24575, 24576, 24577, 100000])
@pytest.mark.parametrize("want,by_mem", [(8192, 1 << 40), (8192, 5000), (2048, 1 << 40)])
@pytest.mark.parametrize("direct", [False, True])
def test_plan_properties_with_the_flag_on(total, want, by_mem, direct):
    cap = min(want, by_mem)
    cap -= cap % 512
    got = _chunks(total, want, by_mem, direct=direct, direct_in=True)
    assert sum(got) == total and min(got) >= 1
    if total < 2048:
        assert got == [total]
        return
    if direct:   # (the copy path's plan puts what its full chunks leave into the last one, above the cap by memory: as ever)
        assert max(got) <= cap, got
    assert max(got) <= max(_chunks(total, want, by_mem, direct=direct)), got   # no chunk larger than the plan without the flag has


def test_an_explicit_plan_still_wins_with_the_flag_on():
    assert _chunks(96, plan="8,16,0,24", direct_in=True) == [8, 16, 1, 24, 47]
    assert _chunks(300, plan="128", direct_in=True) == [128, 172]


def test_the_capability_is_decided_by_shape_alone():
    d = _lib().direct_in
    assert [d(54, 10, 12, 1, b) for b in (1, 256, 16384)] == [1, 1, 1]     # wave1, whatever the batch
    assert d(64, 10, 12, 1, 1) == 1 and d(1, 1, 1, 1, 1) == 1
    assert d(54, 10, 13, 1, 1) == 0 and d(54, 20, 12, 1, 1) == 0           # wave2, wave3: more than one wave per problem
    assert d(54, 10, 12, 2, 1) == 0 and d(65, 10, 12, 1, 1) == 0           # tiled, large-site


def test_the_sources_ride_in_the_row_of_host_addresses():
    """7 problems: one table of 7 pointers (56 -> 256 bytes) for the destinations alone, four tables of 7 (224 -> 256 bytes)
    with the sources; 100 problems: 800 -> 1,024 bytes and 3,200 -> 3,328; the row stays the last of the pinned mirror"""
    o = (ctypes.c_longlong * 7)()
    _lib().host_row(7, 0, 0, o)
    assert o[1] == 0
    _lib().host_row(7, 1, 0, o)
    assert o[1] == 256 and o[2] == o[0] and o[6] == o[0] + 256
    for direct in (0, 1):
        _lib().host_row(7, direct, 1, o)
        assert o[1] == 256 and [o[2 + k] - o[0] for k in range(4)] == [0, 56, 112, 168] and o[6] == o[0] + 256
    _lib().host_row(100, 1, 0, o)
    assert o[1] == 1024
    _lib().host_row(100, 1, 1, o)
    assert o[1] == 3328 and [o[2 + k] - o[0] for k in range(4)] == [0, 800, 1600, 2400] and o[6] == o[0] + 3328
