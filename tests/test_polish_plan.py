"""The polish plan (adacharge_amd/csrc/acn_qp_polplan.hpp: whether a launch is polished and by which kernel, that kernel's
tables, the carve-up of the launch's scratch buffer, the polish launch's grid), compiled for the host as
tests/test_route_table.py compiles the routing table and pinned without a GPU.  The expected values are written out here:
the kind from the rules of DESIGN.md 2.3 / 3.0 and, for the on-chip kind, from tests.polish_cases.polish_tables (the Python
restatement of PolishLds, which this test thereby ties to the header); the scratch offsets from the expressions
acn_qp_api.hip used before there was a plan.  Never computed by the header under test.  The shape's half of the decision --
Route::polish_shape, polish_long_shape, polish_wide_shape -- is read from the routing table, which tests/test_route_table.py
and tests/test_polish_wide_route.py pin."""
import ctypes
import functools
import itertools
import json
import os
import shutil
import subprocess
import tempfile
import types

from tests import polish_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adacharge_amd", "csrc")
INC = os.path.join(ROOT, "include")

SHIM = r"""
#include "acn_qp_polplan.hpp"
using namespace acnqp;
static PolishSwitches switches(int bits) { PolishSwitches s; s.no_polish = bits & 1; s.long_polish = bits & 2; s.wide_polish = bits & 4; return s; }
extern "C" {
// flags: polish_shape, polish_long_shape, polish_wide_shape, tiled of the route; kinds[sw 0..7][iters 0..2][warm 0..1]
void kinds(int N, int M, int cone, int pk, int fl, int mx, int T, int K, const int* iters, int max_iter, int* flags, int* out) {
  const Route r = route_for(site_shape(N, M, cone, pk, fl, mx), T, K, 1, RouteSwitches());
  flags[0] = r.polish_shape; flags[1] = r.polish_long_shape; flags[2] = r.polish_wide_shape; flags[3] = r.tiled;
  for (int sw = 0; sw < 8; ++sw)
    for (int i = 0; i < 3; ++i)
      for (int w = 0; w < 2; ++w) *out++ = (int)polish_plan(r, switches(sw), iters[i], max_iter, w != 0).kind;
}
// out: kind, max_rows, max_sess, blk_doubles, rows_for_solver; tiled < 0: the route's own flag
void plan(int N, int M, int cone, int pk, int T, int K, int tiled, int sw, int iters, int max_iter, int warm, int* out) {
  Route r = route_for(site_shape(N, M, cone, pk, 0, 0), T, K, 1, RouteSwitches());
  if (tiled >= 0) r.tiled = tiled != 0;
  const PolishPlan p = polish_plan(r, switches(sw), iters, max_iter, warm != 0);
  out[0] = (int)p.kind; out[1] = p.max_rows; out[2] = p.max_sess; out[3] = p.blk_doubles; out[4] = p.rows_for_solver;
}
// out: ctr, list, saved, y, slab, total, list_bytes
void scratch(int kind, int batch, int Mg, int Tm, int has_y, long long slab_bytes, long long* out) {
  const PolishScratch s((PolishKind)kind, batch, Mg, Tm, has_y != 0, (size_t)slab_bytes);
  const size_t v[7] = {s.ctr, s.list, s.saved, s.y, s.slab, s.total, s.list_bytes};
  for (int i = 0; i < 7; ++i) out[i] = (long long)v[i];
}
int grid(int kind, int batch, int own, int cus) { return polish_grid((PolishKind)kind, batch, own != 0, cus); }
long long slabs(int kind, int N, int M, int cone, int pk, int T, int K, int grid) {
  return (long long)polish_slab_bytes((PolishKind)kind, site_shape(N, M, cone, pk, 0, 0), T, K, grid);
}
// one workgroup's slab, from the layouts themselves (acn_qp_polslab.hpp, acn_qp_polwide.hpp)
long long long_slab(int N, int T, int K, int Mg, int nrow) { return PolishLongLayout(N, T, K, Mg, nrow).slab_bytes(); }
long long wide_slab(int N, int T, int K, int Mg, int nrow) { return PolishWideLayout(N, T, K, Mg, nrow).slab_bytes(); }
void counters(int* out) { out[0] = kPolCtrPolishQueue; out[1] = kPolCtrResumeQueue; out[2] = kPolCtrListLength; out[3] = kPolCtrRetired; out[4] = (int)PolishScratch::kCtrBytes; }
}
"""

LINEAR, SOC = 0, 1
NONE, ON_CHIP, LONG, WIDE = 0, 1, 2, 3
MAX_ITER = 20000
ITERS = (0, 800, MAX_ITER)
NO_POLISH, LONG_ON, WIDE_ON = 1, 2, 4   # bits of the shim's switches


@functools.lru_cache(maxsize=None)
def _lib():
    tmp = tempfile.mkdtemp(prefix="acnqp_polplan_")
    src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + CSRC, "-I" + INC, src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    shutil.rmtree(tmp)   # (the mapping stays; nothing built is left behind)
    I, LL, PI = ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_int)
    lib.kinds.restype, lib.kinds.argtypes = None, [I] * 8 + [PI, I, PI, PI]
    lib.plan.restype, lib.plan.argtypes = None, [I] * 11 + [PI]
    lib.scratch.restype, lib.scratch.argtypes = None, [I] * 5 + [LL, ctypes.POINTER(LL)]
    lib.grid.restype, lib.grid.argtypes = I, [I] * 4
    lib.slabs.restype, lib.slabs.argtypes = LL, [I] * 8
    lib.long_slab.restype, lib.long_slab.argtypes = LL, [I] * 5
    lib.wide_slab.restype, lib.wide_slab.argtypes = LL, [I] * 5
    lib.counters.restype, lib.counters.argtypes = None, [PI]
    return lib


def _site(N, M, cone, pk, fl=0, mx=0):
    """what polish_cases.polish_tables reads of a site, and the row counts of include/acn_qp.h"""
    return types.SimpleNamespace(N=N, M=M, cone=cone, has_peak=pk, Mg=(2 * M if cone == SOC else M) + pk + fl + mx, nrow=M + pk)


def _plan(N, M, cone, pk, T, K, tiled=-1, sw=0, iters=800, max_iter=MAX_ITER, warm=0):
    out = (ctypes.c_int * 5)()
    _lib().plan(N, M, cone, pk, T, K, tiled, sw, iters, max_iter, warm, out)
    return dict(zip(("kind", "rows", "sess", "blk", "rows_for_solver"), [int(v) for v in out]))


def _long_holds(s, T, K):   # acn_qp_polslab.hpp: the long kernel's thread map and tables
    return 1 <= s.N <= 64 and 33 <= T <= 288 and K >= 1 and s.N * K <= 256 and s.nrow >= 1 and s.nrow <= s.Mg <= 48


def _wide_holds(s, T, K):   # acn_qp_polwide.hpp: the wide kernel's
    return 65 <= s.N <= 1024 and 1 <= T <= 48 and 1 <= K <= 4 and 8 * ((s.N * K + 7) // 8) <= 1024 and s.nrow >= 1 and s.nrow <= s.Mg <= 48


def _expected_kind(s, T, K, flags, sw, iters, warm):
    polish, lng, wide, tiled = flags
    if sw & NO_POLISH or iters <= 0:
        return NONE
    hand_over = iters < MAX_ITER and not warm   # the on-chip and long kinds take over inside the launch, from a cold start
    if polish and hand_over:
        return ON_CHIP if PC.polish_tables(s, T, K, bool(tiled))[2] >= 0 else NONE
    if lng and hand_over and sw & LONG_ON and _long_holds(s, T, K):
        return LONG
    if wide and sw & WIDE_ON and _wide_holds(s, T, K):
        return WIDE
    return NONE


# ---- 1. the kind ---------------------------------------------------------------------------------------------------------
def test_kind_over_shapes_switches_options_and_warm_starts():
    """the shape grid of tests/test_polish_wide_route.py x every combination of the three switches x polish_iters in
    {0, 800, max_iter} x cold / warm"""
    lib, seen = _lib(), {NONE: 0, ON_CHIP: 0, LONG: 0, WIDE: 0}
    iters = (ctypes.c_int * 3)(*ITERS)
    for n in (1, 8, 54, 64, 65, 80, 256, 1024, 1025):
        for t in (1, 12, 16, 17, 24, 32, 33, 48, 49, 144, 288, 289):
            for k in (1, 2, 4, 5):
                for m, cone, pk, fl, mx in ((10, LINEAR, 0, 0, 0), (10, SOC, 1, 0, 0), (0, LINEAR, 1, 0, 0), (20, LINEAR, 0, 1, 0), (31, LINEAR, 0, 0, 1), (24, SOC, 0, 0, 0)):
                    flags, out = (ctypes.c_int * 4)(), (ctypes.c_int * 48)()
                    lib.kinds(n, m, cone, pk, fl, mx, t, k, iters, MAX_ITER, flags, out)
                    s, got = _site(n, m, cone, pk, fl, mx), iter(out)
                    for sw, it, warm in itertools.product(range(8), ITERS, (0, 1)):
                        want, kind = _expected_kind(s, t, k, tuple(flags), sw, it, warm), int(next(got))
                        assert kind == want, (n, t, k, m, cone, pk, fl, mx, sw, it, warm, kind, want)
                        seen[kind] += 1
    assert all(seen.values()), seen


def test_kind_where_the_rules_part():
    short, lng, wide = (54, 10, SOC, 0, 12, 1), (54, 10, SOC, 0, 48, 1), (80, 10, SOC, 0, 12, 1)
    both = LONG_ON | WIDE_ON
    assert [_plan(*s, sw=both)["kind"] for s in (short, lng, wide)] == [ON_CHIP, LONG, WIDE]
    # a warm start: the hand-over kinds do not run, the wide kind does
    assert [_plan(*s, sw=both, warm=1)["kind"] for s in (short, lng, wide)] == [NONE, NONE, WIDE]
    # polish_iters == max_iter (and beyond): likewise; polish_iters == 0: none of them
    assert [_plan(*s, sw=both, iters=MAX_ITER)["kind"] for s in (short, lng, wide)] == [NONE, NONE, WIDE]
    assert [_plan(*s, sw=both, iters=MAX_ITER + 1)["kind"] for s in (short, lng, wide)] == [NONE, NONE, WIDE]
    assert [_plan(*s, sw=both, iters=MAX_ITER - 1)["kind"] for s in (short, lng, wide)] == [ON_CHIP, LONG, WIDE]
    assert [_plan(*s, sw=both, iters=0)["kind"] for s in (short, lng, wide)] == [NONE, NONE, NONE]
    # the handle's switches: a long shape with its switch off is none, whatever the other switch says; the short kind needs none
    assert [_plan(*s, sw=0)["kind"] for s in (short, lng, wide)] == [ON_CHIP, NONE, NONE]
    assert [_plan(*s, sw=WIDE_ON)["kind"] for s in (short, lng, wide)] == [ON_CHIP, NONE, WIDE]
    assert [_plan(*s, sw=LONG_ON)["kind"] for s in (short, lng, wide)] == [ON_CHIP, LONG, NONE]
    # ACNQP_NO_POLISH overrides everything
    for warm in (0, 1):
        assert [_plan(*s, sw=both | NO_POLISH, warm=warm)["kind"] for s in (short, lng, wide)] == [NONE, NONE, NONE]
    # the last shape of the long kind: 64 EVSEs x 4 slots = 256 session columns at horizon 288
    assert _plan(64, 10, SOC, 0, 288, 4, sw=both)["kind"] == LONG and _plan(64, 10, SOC, 0, 289, 4, sw=both)["kind"] == NONE


def test_tables_of_the_slab_kinds():
    # long-horizon: Mg t_max rows, 8 ceil(N K / 8) columns, t_max blocks of Mg (Mg + 1) / 2; the solver gets 8 rows of head room
    p = _plan(54, 10, SOC, 1, 48, 2, sw=LONG_ON)   # Mg = 21, wave5's shape at K = 2: long_ws
    assert p == dict(kind=LONG, rows=21 * 48, sess=112, blk=48 * 21 * 22 // 2, rows_for_solver=21 * 48 + 8), p
    p = _plan(8, 2, LINEAR, 0, 288, 1, sw=LONG_ON)
    assert p == dict(kind=LONG, rows=2 * 288, sess=8, blk=288 * 3, rows_for_solver=2 * 288 + 8), p
    # wide: the long kind's
    p = _plan(130, 6, SOC, 0, 6, 4, sw=WIDE_ON, warm=1)
    assert p == dict(kind=WIDE, rows=12 * 6, sess=520, blk=6 * 12 * 13 // 2, rows_for_solver=12 * 6 + 8), p
    assert _plan(80, 10, SOC, 0, 12, 1, sw=0) == dict(kind=NONE, rows=0, sess=0, blk=0, rows_for_solver=0)


# ---- 2. the on-chip tables against the Python restatement ----------------------------------------------------------------------
def test_on_chip_tables_equal_polish_cases_polish_tables():
    seen, two_per_cu_matters = {ON_CHIP: 0, NONE: 0}, 0
    # (sites of one and of two row tiles under either cone: every one of these shapes is served by an on-chip solver kernel)
    sites = ((LINEAR, 4), (LINEAR, 10), (LINEAR, 20), (SOC, 4), (SOC, 10))
    for n, (cone, m), pk, t, k in itertools.product((1, 8, 54, 64), sites, (0, 1), (1, 12, 16, 17, 24, 32), (1, 2, 4)):
        s = _site(n, m, cone, pk)
        own = _plan(n, m, cone, pk, t, k)
        # (the route's own flag is true wherever two_per_cu asks: horizon <= 16 and one session slot is the wave / tiled family)
        for tiled in ((0, 1) if t <= 16 and k == 1 else (-1,)):
            want = PC.polish_tables(s, t, k, bool(tiled))
            got = _plan(n, m, cone, pk, t, k, tiled=tiled)
            if want[2] < 0:
                assert got == dict(kind=NONE, rows=0, sess=0, blk=0, rows_for_solver=0), (n, cone, pk, t, k, m, tiled, got, want)
            else:
                assert got == dict(kind=ON_CHIP, rows=want[0], sess=want[1], blk=want[2], rows_for_solver=want[0]), (n, cone, pk, t, k, m, tiled, got, want)
            seen[got["kind"]] += 1
            if tiled == 1:
                assert got == own, (n, cone, pk, t, k, m)
                two_per_cu_matters += want != PC.polish_tables(s, t, k, False)
    assert seen[ON_CHIP] > 500 and seen[NONE] > 0 and two_per_cu_matters > 0, (seen, two_per_cu_matters)


# ---- 3. the scratch buffer and the grid ---------------------------------------------------------------------------------------
def _scratch(kind, batch, Mg, Tm, has_y, slab_bytes):
    out = (ctypes.c_longlong * 7)()
    _lib().scratch(kind, batch, Mg, Tm, has_y, slab_bytes, out)
    return dict(zip(("ctr", "list", "saved", "y", "slab", "total", "list_bytes"), [int(v) for v in out]))


def _up(v):
    return (v + 255) & ~255


SCRATCH_SHAPES = {   # kind -> (N, M, cone, peak, t_max, K)
    ON_CHIP: ((54, 10, SOC, 1, 12, 1), (64, 20, LINEAR, 0, 32, 4), (1, 1, LINEAR, 0, 1, 1)),
    LONG: ((54, 10, SOC, 1, 48, 1), (8, 2, SOC, 0, 288, 4), (64, 10, LINEAR, 1, 33, 2)),
    WIDE: ((65, 4, SOC, 0, 8, 1), (130, 6, SOC, 1, 48, 4), (1024, 47, LINEAR, 1, 3, 1)),
}


def test_scratch_offsets_are_the_ones_the_launches_carved_by_hand():
    lib = _lib()
    for kind, shapes in SCRATCH_SHAPES.items():
        for (n, m, cone, pk, t, k), has_y, batch in itertools.product(shapes, (0, 1), (1, 63, 64, 65, 2048)):
            s = _site(n, m, cone, pk)
            # the grid: the slab kernels' caps (32, 16 workgroups); on chip by whose stream it is (test below)
            grid = {ON_CHIP: 0, LONG: max(1, min(batch, 32)), WIDE: max(1, min(batch, 16))}[kind]
            one = {ON_CHIP: 0, LONG: lib.long_slab(n, t, k, s.Mg, s.nrow), WIDE: lib.wide_slab(n, t, k, s.Mg, s.nrow)}[kind]
            if kind != ON_CHIP:
                assert lib.grid(kind, batch, 0, 256) == lib.grid(kind, batch, 1, 256) == grid, (kind, batch)
                assert one > 0 and one % 16 == 0
            sbytes = lib.slabs(kind, n, m, cone, pk, t, k, grid)
            assert sbytes == grid * one, (kind, n, t, k, batch, sbytes, grid, one)
            got = _scratch(kind, batch, s.Mg, t, has_y, sbytes)
            where = (kind, n, t, k, has_y, batch, got)
            # ---- the parent's expressions (acn_qp_api.hip, launch_with_polish and launch_wide_polish) ----
            lbytes = (batch * 4 + 255) & ~255
            ybytes = 0 if has_y else batch * s.Mg * t * 8
            yb256 = (ybytes + 255) & ~255
            assert got["ctr"] == 0 and got["list"] == 256 and got["list_bytes"] == lbytes, where
            if kind == WIDE:
                assert got["saved"] == 256 + lbytes and got["y"] == 256 + 2 * lbytes and got["slab"] == 256 + 2 * lbytes + yb256, where
                assert got["total"] == 256 + 2 * lbytes + yb256 + sbytes, where
            else:
                assert got["y"] == 256 + lbytes and got["saved"] == got["y"], where   # (no saved status: an empty region)
                if kind == LONG:
                    assert got["slab"] == 256 + lbytes + yb256 and got["total"] == 256 + lbytes + yb256 + sbytes, where
                else:   # (the one total that may grow: the multipliers' region is rounded up like the others)
                    assert 256 + lbytes + ybytes <= got["total"] < 256 + lbytes + ybytes + 256, where
            # ---- regions: 256-aligned, in order, disjoint; total is the end of the last; the slab region is the slabs ----
            sizes = [("ctr", 256), ("list", batch * 4), ("saved", batch * 4 if kind == WIDE else 0), ("y", ybytes), ("slab", sbytes)]
            end = 0
            for name, size in sizes:
                assert got[name] % 256 == 0 and got[name] >= end, (name, where)
                end = got[name] + size
            assert got["total"] >= end and got["total"] == _up(end) if kind == ON_CHIP else got["total"] == end, where
            assert got["total"] - got["slab"] == (grid * one if kind != ON_CHIP else 0), where


def test_grid_and_counter_slots():
    g = _lib().grid
    # on chip: one workgroup per CU on a caller's stream, 32 on the handle's own pipeline streams, never more than the problems
    assert [g(ON_CHIP, b, 0, 256) for b in (1, 31, 32, 33, 255, 256, 257, 4096)] == [1, 31, 32, 33, 255, 256, 256, 256]
    assert [g(ON_CHIP, b, 1, 256) for b in (1, 31, 32, 33, 4096)] == [1, 31, 32, 32, 32]
    assert g(ON_CHIP, 4096, 0, 304) == 304 and g(ON_CHIP, 0, 0, 256) == 1
    assert [g(LONG, b, own, 256) for b in (0, 1, 31, 32, 33, 4096) for own in (0, 1)] == [1, 1, 1, 1, 31, 31, 32, 32, 32, 32, 32, 32]
    assert [g(WIDE, b, own, 256) for b in (0, 1, 15, 16, 17, 4096) for own in (0, 1)] == [1, 1, 1, 1, 15, 15, 16, 16, 16, 16, 16, 16]
    out = (ctypes.c_int * 5)()
    _lib().counters(out)
    # [0] the polish kernel's queue, [1] the resume launch's, [2] the list length, [3] the solver's retired count; one 256-byte line
    assert list(out) == [0, 1, 2, 3, 256]


# ---- 4. the carve-up under a sanitizer ------------------------------------------------------------------------------------------
def test_scratch_carve_up_under_address_sanitizer(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++")) if c), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "polish_scratch")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + INC,
                    os.path.join(ROOT, "tests", "host", "polish_scratch.cpp"), "-o", exe], check=True, timeout=180)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"[polish-plan] {out['combinations']} carve-ups, the largest {out['largest_total']} bytes; by kind {out['by_kind']}")
    assert out["failures"] == 0 and out["combinations"] >= 1000 and all(n > 200 for n in out["by_kind"]), out
