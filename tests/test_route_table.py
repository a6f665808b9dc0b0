"""The routing table (adacharge_amd/csrc/acn_qp_route.hpp) and the chunk planner (acn_qp_pipeline.hpp), compiled for the
host (g++, as tests/test_check_rules.py compiles the check rules) and pinned without a GPU.  The expected values are
written out here from DESIGN.md section 3 and from what tests/golden/edges.npz declares, never computed by the headers.
The kernels' own size formulas are replaced by recognisable numbers (the shim's `Fake`), so that the test sees WHICH
formula the table asks and with which arguments."""
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adacharge_amd", "csrc")
INC = os.path.join(ROOT, "include")

SHIM = r"""
#include "acn_qp_route.hpp"
#include "acn_qp_pipeline.hpp"
using namespace acnqp;
struct Fake {
  static int wave_accel() { return 6; }
  static int tiled_accel(int MT, int CT, int NP, int K) { return 3; }
  static int stream_accel() { return 5; }
  static int long_accel() { return 4; }
  static int general_accel() { return 2; }
  static long long stream_workspace(int NP, int CT, int K, int MT, int accel) { return 1000000000LL + NP * 100000LL + CT * 10000 + K * 1000 + MT * 100 + accel; }
  static long long long_workspace(int NP, int t_max, int K, int MT, int accel) { return 2000000000LL + NP * 100000LL + t_max * 100 + K * 10000000LL + MT * 10 + accel; }
};
static RouteSwitches sw(const int* s) { RouteSwitches r; r.no_wave = s[0]; r.no_wave2 = s[1]; r.wave_min_batch = s[2]; r.no_long = s[3]; r.lds_long = s[4]; return r; }
extern "C" {
int padded(int cone, int M, int pk, int fl, int mx) { return padded_rows(cone, M, pk, fl, mx); }
// out: family, wv, tiled, stream, lng, lds, on_chip, polish_shape, chunk_want, accel_cap, MR, Mg, NP, long_shape
void route(int N, int M, int cone, int pk, int fl, int mx, int T, int K, int batch, const int* s, long long* out, long long* ws, int accel_req) {
  const SiteShape site = site_shape(N, M, cone, pk, fl, mx);
  const Route r = route_for(site, T, K, batch, sw(s));
  const long long v[14] = {r.family, r.wv, r.tiled, r.stream, r.lng, r.lds, r.on_chip, r.polish_shape, r.chunk_want(), r.accel_cap<Fake>(),
                           site.MR, site.Mg, site.NP(), long_shape(site, T, K, sw(s))};
  for (int i = 0; i < 14; ++i) out[i] = v[i];
  *ws = r.workspace_doubles<Fake>(accel_req);
}
int any_batch() { return kRouteAnyBatch; }
long long by_memory(long long N, long long T, long long K) { return chunk_cap_by_memory(N, T, K); }
// the chunk sizes of a one-shape call, as the chunk loop realises the planner's caps
int chunks(long long total, long long want, long long by_mem, int wave, int uniform, long long chunk, const char* plan, int ramp, long long* out, int n) {
  PlanEnv env; env.chunk = chunk; env.plan = plan; env.ramp = ramp;
  const std::vector<long long> caps = plan_chunk_caps(total, want, by_mem, wave, uniform, env);
  int c = 0;
  for (long long lo = 0; lo < total && c < n; ++c) { out[c] = std::min(total - lo, chunk_cap(caps, c)); lo += out[c]; }
  return c;
}
}
"""

LINEAR, SOC = 0, 1
NAMES = {1: "wave1", 2: "wave2", 3: "wave3", 4: "wave4", 5: "wave5", 6: "tiled_ct1", 7: "tiled_ct2", 8: "long_lds", 9: "long_ws",
         10: "stream", 11: "general"}
DEFAULT = (0, 0, 1, 0, 1)   # no_wave, no_wave2, wave_min_batch, no_long, lds_long


@functools.lru_cache(maxsize=None)
def _lib():
    tmp = tempfile.mkdtemp(prefix="acnqp_route_")
    src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.run([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-I" + INC, src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    shutil.rmtree(tmp)   # (the mapping stays; nothing built is left behind)
    LL, I = ctypes.c_longlong, ctypes.c_int
    lib.padded.restype, lib.padded.argtypes = I, [I] * 5
    lib.route.restype, lib.route.argtypes = None, [I] * 9 + [ctypes.POINTER(I), ctypes.POINTER(LL), ctypes.POINTER(LL), I]
    lib.by_memory.restype, lib.by_memory.argtypes = LL, [LL] * 3
    lib.chunks.restype, lib.chunks.argtypes = I, [LL, LL, LL, I, I, LL, ctypes.c_char_p, I, ctypes.POINTER(LL), I]
    return lib


def _route(N, M, T, K, batch=1, cone=LINEAR, pk=0, fl=0, mx=0, sw=DEFAULT, accel=5):
    out, ws = (ctypes.c_longlong * 14)(), ctypes.c_longlong(0)
    _lib().route(N, M, cone, pk, fl, mx, T, K, batch, (ctypes.c_int * 5)(*sw), out, ctypes.byref(ws), accel)
    keys = ("family", "wv", "tiled", "stream", "lng", "lds", "on_chip", "polish", "want", "accel", "MR", "Mg", "NP", "long_shape")
    r = dict(zip(keys, [int(v) for v in out]))
    r["ws"] = int(ws.value)
    r["name"] = NAMES[r["family"]]
    return r


def _chunks(total, want, by_mem=1 << 40, wave=False, uniform=True, chunk=0, plan=None, ramp=True):
    out = (ctypes.c_longlong * 64)()
    n = _lib().chunks(total, want, by_mem, int(wave), int(uniform), chunk, None if plan is None else plan.encode(), int(ramp), out, 64)
    return [int(out[i]) for i in range(n)]


# ---- the site's padded rows ---------------------------------------------------------------------------------------------
def test_padded_rows_against_what_acnqp_create_accepts_and_refuses():
    p = _lib().padded
    assert [p(LINEAR, m, 0, 0, 0) for m in (0, 16, 17, 48, 49)] == [0, 16, 17, 48, 49]   # acnqp_create refuses the last
    assert p(LINEAR, 47, 1, 0, 0) == 48 and p(LINEAR, 47, 1, 1, 0) == 49 and p(LINEAR, 45, 1, 1, 1) == 48
    assert [p(SOC, m, 0, 0, 0) for m in (1, 4, 5, 10, 21, 24, 25)] == [8, 8, 16, 24, 48, 48, 56]   # 21 accepted, 25 refused
    assert p(SOC, 21, 1, 0, 0) == 49 and p(SOC, 20, 1, 1, 1) == 43
    # ... rounded up to whole 16-row tiles, never fewer than one
    assert [_route(8, m, 12, 1)["MR"] for m in (0, 1, 16, 17, 32, 33, 48)] == [16, 16, 16, 32, 32, 48, 48]
    assert _route(54, 10, 12, 1, cone=SOC, pk=1)["MR"] == 32 and _route(54, 10, 12, 1, cone=SOC, pk=1)["Mg"] == 21
    assert [_route(n, 4, 12, 1)["NP"] for n in (1, 64, 65, 80, 81, 1023)] == [64, 64, 80, 80, 96, 1024]


# ---- families -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [str(n) for n in H.load_edges()["names"]])
def test_family_of_every_edge_fixture(name):
    from adacharge_amd.builder import build_batch

    sl, infra, iface, obj, meta, peak, exp = H.edges_case(H.load_edges(), name)
    batch = build_batch([sl], infra, iface, obj, meta["ct"], meta["eq"], peak_limits=[peak])
    s = batch.site
    r = _route(s.N, s.M, batch.Tm, batch.K, 1, cone=int(s.cone), pk=int(s.has_peak), fl=int(s.has_flat), mx=int(s.has_max))
    assert r["name"] == meta["family"], (name, r)


# (N, infrastructure rows of a LINEAR site, t_max, k_sessions) -> family.  10 / 20 / 40 rows: one / two / three row tiles.
CUTS = [
    ((64, 10, 12, 1), "wave1"), ((65, 10, 12, 1), "stream"),                                # N 64 / 65
    ((54, 10, 12, 1), "wave1"), ((54, 10, 13, 1), "wave2"),                                 # horizon 12 / 13
    ((54, 10, 24, 1), "wave2"), ((54, 10, 25, 1), "tiled_ct2"),                             # 24 / 25
    ((54, 10, 32, 1), "tiled_ct2"), ((54, 10, 33, 1), "wave5"),                             # 32 / 33
    ((54, 10, 48, 1), "wave5"), ((54, 10, 49, 1), "long_ws"),                               # 48 / 49
    ((54, 10, 288, 1), "long_ws"), ((54, 10, 289, 1), "general"),                           # 288 / 289
    ((54, 10, 16, 2), "tiled_ct1"), ((54, 10, 17, 2), "tiled_ct2"),                         # 16 / 17, one row tile
    ((54, 20, 16, 2), "tiled_ct1"), ((54, 20, 17, 2), "long_lds"),                          # ... two row tiles
    ((54, 16, 12, 1), "wave1"), ((54, 17, 12, 1), "wave3"),                                 # 16 / 17 padded rows
    ((54, 20, 13, 1), "wave4"), ((54, 20, 24, 1), "wave4"), ((54, 20, 25, 1), "long_lds"),
    ((54, 32, 24, 1), "wave4"), ((54, 33, 24, 1), "general"),                               # 32 / 33 padded rows
    ((54, 40, 12, 1), "tiled_ct1"), ((54, 40, 16, 4), "tiled_ct1"), ((54, 40, 17, 1), "general"),
    ((54, 20, 32, 1), "long_lds"), ((54, 20, 33, 1), "long_ws"),
    ((54, 10, 12, 2), "tiled_ct1"),                                                         # one against two session slots
    ((54, 10, 12, 4), "tiled_ct1"), ((54, 10, 12, 5), "long_ws"),                           # four against five
    ((54, 10, 24, 4), "tiled_ct2"), ((54, 10, 24, 5), "long_ws"),
    ((65, 10, 48, 1), "stream"), ((65, 10, 49, 1), "long_ws"), ((128, 40, 49, 1), "general"), ((1024, 10, 48, 5), "stream"),
]


@pytest.mark.parametrize("shape,family", CUTS)
def test_cut_points(shape, family):
    assert _route(*shape)["name"] == family


def test_a_demand_charge_row():
    assert _route(54, 32, 24, 2)["name"] == "long_lds" and _route(54, 31, 24, 2, mx=1)["name"] == "long_ws"   # both 32 padded rows
    assert _route(54, 10, 12, 1, mx=1)["name"] == "wave1" and _route(54, 10, 12, 2, mx=1)["name"] == "tiled_ct1"


# ---- the quirks, as facts of the table -----------------------------------------------------------------------------------
def test_accel_columns_ask_as_if_the_batch_were_unbounded():
    sw = (0, 0, 4096, 0, 1)   # ACNQP_WAVE_MIN_BATCH=4096
    any_batch = _lib().any_batch()
    assert any_batch == 1 << 30
    assert _route(54, 10, 12, 1, batch=100, sw=sw)["accel"] == 3     # (what a launch of 100 runs: the tiled kernel)
    assert _route(54, 10, 12, 1, batch=any_batch, sw=sw)["accel"] == 6   # what acnqp_accel_columns asks: the wave kernel's
    assert [_route(*s)["accel"] for s in ((65, 10, 12, 1), (54, 10, 96, 1), (54, 10, 300, 1), (54, 10, 16, 2))] == [5, 4, 2, 3]


def test_chunk_size_wanted():
    assert _route(54, 10, 12, 1)["want"] == 8192 and _route(54, 10, 12, 2)["want"] == 1024 and _route(54, 10, 96, 1)["want"] == 2048
    assert _route(65, 10, 12, 1)["want"] == 2048 and _route(54, 10, 300, 1)["want"] == 2048
    lds = _route(54, 20, 24, 2)
    assert lds["name"] == "long_lds" and lds["on_chip"] == 1 and lds["want"] == 2048
    w5 = _route(54, 10, 40, 1)
    assert w5["name"] == "wave5" and w5["tiled"] == 1 and w5["want"] == 8192
    assert _route(54, 10, 40, 1, sw=(1, 0, 1, 0, 1))["want"] == 2048   # ... the same shape without the wave kernel: not tiled_shape


def test_a_wave5_shape_is_a_long_shape_and_still_routed_to_the_wave_kernel():
    r = _route(54, 10, 40, 1)
    assert r["long_shape"] == 1 and r["name"] == "wave5" and r["lng"] == 0
    assert _route(54, 10, 40, 1, sw=(0, 1, 1, 0, 1))["name"] == "long_ws"


def test_polish_eligibility():
    assert _route(54, 10, 12, 1)["polish"] == 1 and _route(54, 10, 32, 4, pk=1)["polish"] == 1 and _route(54, 20, 24, 2)["polish"] == 1
    assert _route(54, 10, 12, 1, fl=1)["polish"] == 0 and _route(54, 10, 12, 1, mx=1)["polish"] == 0
    assert _route(54, 10, 33, 1)["polish"] == 0 and _route(54, 10, 12, 5)["polish"] == 0 and _route(65, 10, 12, 1)["polish"] == 0
    assert _route(54, 0, 12, 1)["polish"] == 0 and _route(54, 0, 12, 1, pk=1)["polish"] == 1   # no site row at all
    assert _route(54, 31, 24, 2, mx=1)["polish"] == 0   # long_ws: not on chip


def test_workspace_per_workgroup():
    assert _route(54, 10, 12, 1)["ws"] == 0 and _route(54, 10, 32, 4)["ws"] == 0 and _route(54, 10, 40, 1)["ws"] == 0
    # large-site kernel: (NP, column tiles, K, row tiles, min(requested, its ring))
    assert _route(65, 20, 40, 2, accel=9)["ws"] == 1000000000 + 80 * 100000 + 3 * 10000 + 2 * 1000 + 2 * 100 + 5
    assert _route(65, 20, 40, 2, accel=-3)["ws"] == 1000000000 + 80 * 100000 + 3 * 10000 + 2 * 1000 + 2 * 100 + 0
    # long-horizon kernel: (NP, t_max, K, row tiles, min(requested, its ring)), LDS-resident or not
    assert _route(54, 20, 96, 1, accel=9)["ws"] == 2000000000 + 64 * 100000 + 96 * 100 + 10000000 + 2 * 10 + 4
    assert _route(54, 20, 24, 2, accel=3)["ws"] == 2000000000 + 64 * 100000 + 24 * 100 + 2 * 10000000 + 2 * 10 + 3
    # general-shape kernel, 54 x 300, 16 padded rows, two columns: n = 16,200, mt = 4,800
    assert _route(54, 10, 300, 1, accel=5)["ws"] == 7 * 16200 + 8 * 4800 + 3 * 54 + 8 + 2 * 21000 + (5 * 21000 * 4 + 7) // 8 + 2 == 246472


# ---- the diagnostic switches -----------------------------------------------------------------------------------------------
def test_switches():
    assert _route(54, 10, 12, 1, sw=(1, 0, 1, 0, 1))["name"] == "tiled_ct1"            # NO_WAVE: the headline shape
    no2 = (0, 1, 1, 0, 1)                                                                # NO_WAVE2: variant 1 stays
    assert [_route(*s, sw=no2)["name"] for s in ((54, 10, 12, 1), (54, 10, 13, 1), (54, 20, 12, 1), (54, 20, 24, 1), (54, 10, 40, 1))] == \
        ["wave1", "tiled_ct1", "tiled_ct1", "long_lds", "long_ws"]
    mb = (0, 0, 100, 0, 1)                                                               # WAVE_MIN_BATCH: on `batch` only
    assert _route(54, 10, 12, 1, batch=99, sw=mb)["name"] == "tiled_ct1" and _route(54, 10, 12, 1, batch=100, sw=mb)["name"] == "wave1"
    assert _route(54, 10, 12, 2, batch=99, sw=mb)["name"] == _route(54, 10, 12, 2, batch=100, sw=mb)["name"] == "tiled_ct1"
    assert _route(54, 10, 144, 1)["name"] == "long_ws" and _route(54, 10, 144, 1, sw=(0, 0, 1, 1, 1))["name"] == "general"   # NO_LONG
    jpl = dict(cone=SOC)                                                                 # jpl52: 10 SOC rows -> 24 -> two row tiles
    assert _route(52, 10, 24, 2, **jpl)["name"] == "long_lds" and _route(52, 10, 24, 2, sw=(0, 0, 1, 0, 0), **jpl)["name"] == "long_ws"


# ---- the planner -----------------------------------------------------------------------------------------------------------
def test_planner():
    assert _chunks(16384, 8192, wave=True) == [2048, 4096, 8192, 2048]
    assert _chunks(2047, 8192, wave=True) == [2047]
    assert _chunks(4096, 8192, wave=True) == [1024, 2048, 1024]
    assert _chunks(4000, 1024) == [256, 512, 1024, 1024, 1024, 160]
    assert _chunks(1800, 1024) == [256, 512, 1024, 8]
    assert _chunks(16384, 8192, wave=True, uniform=False) == [2048, 4096, 8192, 2048]   # not planned: the ramp, by chance the same
    assert _chunks(20000, 8192, wave=True, uniform=False) == [2048, 4096, 8192, 5664] and _chunks(20000, 8192, wave=True) == [1664, 3328, 6656, 6656, 1696]   # c = 6,656: 20,000 / 3 in whole rounds
    assert _chunks(96, 8192, wave=True, plan="8,16,0,24") == [8, 16, 1, 24, 47]          # an entry below 1 is clamped
    assert _chunks(96, 8192, wave=True, plan="8,16,8,24,8") == [8, 16, 8, 24, 8, 32]
    assert _chunks(96, 1024, plan="8,16") == [96]                                        # (only planned calls read it)
    assert _chunks(100, 1024, chunk=24) == [24, 24, 24, 24, 4] and _chunks(100, 2048, chunk=24, uniform=False) == [24, 24, 24, 24, 4]
    assert _chunks(4000, 1024, ramp=False) == [1024, 1024, 1024, 928]
    assert _chunks(3000, 1300) == [256, 512, 1024, 1024, 184]                            # whole rounds of 512 slots
    # 1 GiB of staging per chunk: 1,024 EVSEs x 4,096 periods stage 134,266,976 bytes per problem
    assert _lib().by_memory(1024, 4096, 1) == 7 and _chunks(20, 2048, by_mem=7) == [7, 7, 6]
    assert _lib().by_memory(54, 12, 1) == (1 << 30) // (4 * 54 * 12 * 8 + 54 * 16 + 12 * 8 + 96)
