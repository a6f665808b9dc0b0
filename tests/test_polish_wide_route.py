"""``Route::polish_wide_shape`` (adacharge_amd/csrc/acn_qp_route.hpp), compiled for the host as tests/test_route_table.py
compiles the routing table and pinned without a GPU: the shapes the wide-site polish serves (acn_qp_polish_wide.hpp), that
it is never true together with the other two polish flags, and that those two are what they were on the shapes
tests/test_route_table.py pins.  The expected values are written out here from the issue's list, never computed by the header."""
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adacharge_amd", "csrc")
INC = os.path.join(ROOT, "include")

SHIM = r"""
#include "acn_qp_route.hpp"
#include "acn_qp_polwide.hpp"
using namespace acnqp;
extern "C" {
// out: family, polish_shape, polish_long_shape, polish_wide_shape, polish_wide_holds
void route(int N, int M, int cone, int pk, int fl, int mx, int T, int K, int batch, int* out) {
  const SiteShape site = site_shape(N, M, cone, pk, fl, mx);
  const Route r = route_for(site, T, K, batch, RouteSwitches());
  out[0] = r.family; out[1] = r.polish_shape; out[2] = r.polish_long_shape; out[3] = r.polish_wide_shape;
  out[4] = polish_wide_holds(N, T, K, site.Mg, M + (pk ? 1 : 0));
}
}
"""

LINEAR, SOC = 0, 1
STREAM = 10


@functools.lru_cache(maxsize=None)
def _lib():
    tmp = tempfile.mkdtemp(prefix="acnqp_wide_route_")
    src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.run([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-I" + INC, src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    shutil.rmtree(tmp)   # (the mapping stays; nothing built is left behind)
    lib.route.restype, lib.route.argtypes = None, [ctypes.c_int] * 9 + [ctypes.POINTER(ctypes.c_int)]
    return lib


def _route(N, M, T, K, batch=1, cone=LINEAR, pk=0, fl=0, mx=0):
    out = (ctypes.c_int * 5)()
    _lib().route(N, M, cone, pk, fl, mx, T, K, batch, out)
    return dict(zip(("family", "polish", "long", "wide", "holds"), [int(v) for v in out]))


def test_wide_shape_is_the_stream_family_up_to_1024_evses_and_1024_session_columns():
    for n in (65, 1024):
        for t in (1, 48):
            for cone in (LINEAR, SOC):
                r = _route(n, 10, t, 1, cone=cone)
                assert r == dict(family=STREAM, polish=0, long=0, wide=1, holds=1), (n, t, cone, r)
    assert _route(256, 10, 12, 4)["wide"] == 1 and _route(72, 5, 12, 4, cone=SOC, pk=1)["wide"] == 1
    assert _route(1024, 24, 48, 1, cone=SOC)["wide"] == 1 and _route(1024, 47, 48, 1, pk=1)["wide"] == 1   # 48 rows at the ABI
    assert _route(80, 0, 12, 1, pk=1)["wide"] == 1                                                       # the peak row alone


def test_wide_shape_is_false_outside_them():
    assert _route(64, 10, 12, 1)["wide"] == 0 and _route(64, 10, 48, 1)["wide"] == 0       # N 64: the other kernels' sites
    assert _route(65, 10, 49, 1)["wide"] == 0 and _route(1024, 10, 49, 1)["wide"] == 0     # t_max 49: not the stream family
    assert _route(80, 10, 12, 1, fl=1)["wide"] == 0 and _route(80, 10, 12, 1, mx=1)["wide"] == 0   # a flat or max row
    assert _route(80, 10, 12, 1, pk=1, fl=1, mx=1)["wide"] == 0
    assert _route(257, 10, 12, 4)["wide"] == 0 and _route(513, 10, 12, 2)["wide"] == 0 and _route(1024, 10, 12, 2)["wide"] == 0   # N K beyond 1,024
    assert _route(342, 10, 12, 3)["wide"] == 0 and _route(341, 10, 12, 3)["wide"] == 1     # 8 ceil(N K / 8): 1,032 | 1,024 columns
    assert _route(80, 10, 12, 5)["wide"] == 0                                             # a fifth session slot
    assert _route(80, 0, 12, 1)["wide"] == 0                                              # a site with no row
    assert _route(1025, 10, 12, 1)["wide"] == 0                                           # beyond the tables
    for r in (_route(64, 10, 12, 1), _route(80, 10, 12, 5), _route(257, 10, 12, 4), _route(80, 0, 12, 1), _route(1025, 10, 12, 1), _route(65, 10, 49, 1)):
        assert r["holds"] == 0 or r["family"] != STREAM, r   # what the route refuses by shape, the kernel's own predicate refuses too


def test_no_shape_has_two_polish_flags_and_the_other_two_are_what_they_were():
    # polish_shape / polish_long_shape on the shapes tests/test_route_table.py pins
    assert _route(54, 10, 12, 1)["polish"] == 1 and _route(54, 10, 32, 4, pk=1)["polish"] == 1 and _route(54, 20, 24, 2)["polish"] == 1
    assert _route(54, 10, 12, 1, fl=1)["polish"] == 0 and _route(54, 10, 12, 1, mx=1)["polish"] == 0
    assert _route(54, 10, 33, 1)["polish"] == 0 and _route(54, 10, 12, 5)["polish"] == 0 and _route(65, 10, 12, 1)["polish"] == 0
    assert _route(54, 0, 12, 1)["polish"] == 0 and _route(54, 0, 12, 1, pk=1)["polish"] == 1
    assert _route(54, 31, 24, 2, mx=1)["polish"] == 0
    assert _route(54, 10, 33, 1)["long"] == 1 and _route(54, 10, 288, 4)["long"] == 1 and _route(54, 10, 289, 1)["long"] == 0
    assert _route(54, 10, 32, 1)["long"] == 0 and _route(65, 10, 48, 1)["long"] == 0 and _route(54, 10, 48, 1, fl=1)["long"] == 0
    for n in (1, 8, 54, 64, 65, 80, 256, 1024, 1025):
        for t in (1, 12, 16, 17, 24, 32, 33, 48, 49, 144, 288, 289):
            for k in (1, 2, 4, 5):
                for m, cone, pk, fl, mx in ((10, LINEAR, 0, 0, 0), (10, SOC, 1, 0, 0), (0, LINEAR, 1, 0, 0), (20, LINEAR, 0, 1, 0), (31, LINEAR, 0, 0, 1), (24, SOC, 0, 0, 0)):
                    r = _route(n, m, t, k, cone=cone, pk=pk, fl=fl, mx=mx)
                    assert r["polish"] + r["long"] + r["wide"] <= 1, (n, t, k, m, cone, pk, fl, mx, r)
                    assert r["wide"] == 0 or (r["family"] == STREAM and r["holds"] == 1), (n, t, k, r)
