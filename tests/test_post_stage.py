"""The host-only part of adacharge_amd/csrc/acn_qp_post.hpp -- the table row of a staged array, the planner of the
post-solve host entries (acnqp_duals_host, acnqp_pilots_host, acnqp_advance_host) and the overlap predicate of their
argument checks -- compiled for the host (g++, as tests/test_route_table.py compiles the routing table) and pinned
without a GPU.  Every expected value is written out here; the byte tables of the three entries are written out from
include/acn_qp.h, never taken from the header under test."""
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
#include "acn_qp_post.hpp"
using namespace acnqp;
extern "C" {
long long budget() { return (long long)kPostBudget; }
// row k: bytes[k], whole[k].  offs[k]: its staging offset (-1: none), addr[k]: its staging address in a buffer at `base`
// (0: null); out: chunk, need.  capped == 0: the call of a run without ACNQP_POST_CHUNK.
void plan(int n, const long long* bytes, const int* whole, long long batch, long long budget, int capped, long long cap,
          long long base, long long* offs, long long* addr, long long* out) {
  std::vector<Staged> a;
  for (int k = 0; k < n; ++k) a.push_back(whole[k] ? Staged::plan(nullptr, (size_t)bytes[k]) : Staged::in(nullptr, (size_t)bytes[k]));
  const StagePlan pl = capped ? plan_stage(a.data(), n, (size_t)batch, (size_t)budget, cap) : plan_stage(a.data(), n, (size_t)batch, (size_t)budget);
  for (int k = 0; k < n; ++k) {
    offs[k] = pl.offs[k] == StagePlan::kNone ? -1 : (long long)pl.offs[k];
    const char* p = pl.at(reinterpret_cast<char*>(base), k);
    addr[k] = (long long)reinterpret_cast<size_t>(p);
  }
  out[0] = (long long)pl.chunk; out[1] = (long long)pl.need;
}
// the row helpers: src, dst, whole of Staged::plan / in / out of the address p
void rows(long long p, long long* out) {
  void* q = reinterpret_cast<void*>(p);
  const Staged r[3] = {Staged::plan(q, 5), Staged::in(q, 6), Staged::out(q, 7)};
  for (int k = 0; k < 3; ++k) { out[4 * k] = (long long)reinterpret_cast<size_t>(r[k].src); out[4 * k + 1] = (long long)reinterpret_cast<size_t>(r[k].dst);
                                out[4 * k + 2] = (long long)r[k].bytes; out[4 * k + 3] = r[k].whole; }
}
int meet(long long p, long long np, long long q, long long nq) {
  return spans_meet(reinterpret_cast<const void*>(p), (size_t)np, reinterpret_cast<const void*>(q), (size_t)nq);
}
}
"""

BUDGET = 256 << 20


@functools.lru_cache(maxsize=None)
def _lib():
    tmp = tempfile.mkdtemp(prefix="acnqp_post_")
    src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.run([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-I" + INC, src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    shutil.rmtree(tmp)   # (the mapping stays; nothing built is left behind)
    LL, I, P = ctypes.c_longlong, ctypes.c_int, ctypes.POINTER
    lib.budget.restype, lib.budget.argtypes = LL, []
    lib.plan.restype, lib.plan.argtypes = None, [I, P(LL), P(I), LL, LL, I, LL, LL, P(LL), P(LL), P(LL)]
    lib.rows.restype, lib.rows.argtypes = None, [LL, P(LL)]
    lib.meet.restype, lib.meet.argtypes = I, [LL] * 4
    return lib


def _plan(rows, batch, budget=BUDGET, cap=None, base=1 << 20):
    """rows: ("whole" | "per", bytes).  -> (chunk, need, offsets with None for an array without room); the addresses the
    plan reports are checked against the offsets on the way"""
    n = len(rows)
    LL = ctypes.c_longlong
    offs, addr, out = (LL * n)(), (LL * n)(), (LL * 2)()
    _lib().plan(n, (LL * n)(*[b for _, b in rows]), (ctypes.c_int * n)(*[int(w == "whole") for w, _ in rows]), batch, budget,
                int(cap is not None), cap or 0, base, offs, addr, out)
    for k in range(n):
        assert addr[k] == (0 if offs[k] < 0 else base + offs[k]), k   # no room: no address
    return int(out[0]), int(out[1]), [None if o < 0 else int(o) for o in offs]


def _chunks(batch, chunk):
    """the chunk loop of run_staged: for (lo = 0; lo < batch; lo += chunk) nb = min(chunk, batch - lo)"""
    return [min(chunk, batch - lo) for lo in range(0, batch, chunk)]


def per(*b):
    return [("per", x) for x in b]


def whole(*b):
    return [("whole", x) for x in b]


# ---- the table row ------------------------------------------------------------------------------------------------------
def test_row_helpers():
    out = (ctypes.c_longlong * 12)()
    _lib().rows(4096, out)
    assert list(out) == [4096, 0, 5, 1,   4096, 0, 6, 0,   0, 4096, 7, 0]   # plan: uploaded, whole; in: uploaded; out: downloaded
    assert _lib().budget() == 268435456


# ---- the chunk ------------------------------------------------------------------------------------------------------------
def test_chunk_by_budget():
    one = per(1000)
    assert _plan(one, 10, budget=10000)[0] == 10          # the budget holds all problems
    assert _plan(one, 25, budget=10000)[0] == 10          # ... ten of them
    assert _plan(one, 10, budget=1000)[0] == 1            # exactly one
    assert _plan(one, 10, budget=999)[0] == 1             # less than one: still one
    assert _plan(per(600, 0, 400), 25, budget=10999)[0] == 10   # the SUM of the per-problem bytes
    assert _plan(whole(5000) + one, 25, budget=10000)[0] == 10  # a whole-call array is not charged to the chunk


def test_zero_per_problem_total():
    assert _plan(whole(64) + per(0), 5) == (5, 256, [0, None])
    assert _plan(per(0, 0), 3) == (3, 0, [None, None])


def test_cap():
    one = per(1000)
    assert [_plan(one, 25, budget=10000, cap=c)[0] for c in (9, 10, 11)] == [9, 10, 10]   # below, equal to, above the budget's chunk
    assert [_plan(one, 25, budget=10000, cap=c)[0] for c in (0, -5)] == [1, 1]
    assert _plan(one, 25, budget=10000, cap=None)[0] == 10
    assert _plan(one, 7, cap=3)[0] == 3 and _chunks(7, 3) == [3, 3, 1]
    assert _chunks(6, 4) == [4, 2] and _chunks(4, 3) == [3, 1] and _chunks(7, 7) == [7] and _chunks(7, 1) == [1] * 7


# ---- the offsets ------------------------------------------------------------------------------------------------------------
def test_offsets():
    rows = per(100) + whole(300) + per(0) + per(8) + whole(0) + whole(256)
    chunk, need, offs = _plan(rows, 10, budget=10000)
    assert chunk == 10                                     # 10,000 / 108 = 92 > the batch
    # whole-call arrays first (300 -> 512, 256 -> 256), then 10 x 100 -> 1,024 and 10 x 8 -> 256
    assert offs == [768, 0, None, 1792, None, 512] and need == 2048 == 1792 + 256
    assert all(o % 256 == 0 for o in offs if o is not None)
    # a smaller chunk moves the per-problem arrays only: 3 x 100 -> 512, 3 x 8 -> 256
    assert _plan(rows, 10, budget=10000, cap=3) == (3, 1536, [768, 0, None, 1280, None, 512])


# ---- the three entries' own tables (bytes per problem / per array: include/acn_qp.h) ----------------------------------
NV = 54 * 12 * 8   # a (N, Tm) array of doubles: 5,184 bytes


def test_duals_table_54x12_k1_one_peak_row():
    """caltech54 SOC with a peak row (Mg = 21), K = 1, status and z given: lb ub q x y s_off s_len s_cap peak horizon pdiag
    s_eq lf dc status | mu z res"""
    rows = per(NV, NV, NV, NV, 21 * 12 * 8, 54 * 4, 54 * 4, 54 * 8, 12 * 8, 4, 8, 1, 0, 0, 4, 54 * 8, NV, 32)
    assert sum(b for _, b in rows) == 29377
    chunk, need, offs = _plan(rows, 16384)
    assert chunk == 9137 == BUDGET // 29377 and need == 268419840 and _chunks(16384, chunk) == [9137, 7247]
    chunk, need, offs = _plan(rows, 6)
    assert (chunk, need) == (6, 179200)
    assert offs == [0, 31232, 62464, 93696, 124928, 137216, 138752, 140288, 143104, 143872, 144128, 144384, None, None, 144640,
                    144896, 147712, 178944]
    assert need == offs[-1] + 256
    chunk, need, offs = _plan(rows, 6, cap=4)
    assert (chunk, need) == (4, 119296) and offs[1] == 20736 and offs[12:15] == [None, None, 96256] and offs[-1] == 119040


def test_pilots_table_reallocate():
    """REALLOCATE, 64 x 54 x 12, 10 infrastructure rows, 26 levels, 70 sessions, every output: cre cim limits max_pilot
    levels sess_seg s_evse s_arrived s_cap | x | pilots first visits"""
    rows = whole(10 * 54 * 8, 10 * 54 * 8, 10 * 8, 0, 54 * 26 * 8, 65 * 4, 70 * 4, 70, 70 * 8) + per(NV, NV, 54 * 8, 4)
    chunk, need, offs = _plan(rows, 64)
    assert (chunk, need) == (64, 713728)                   # 10,804 bytes per problem: 24,845 fit
    assert offs == [0, 4352, 8704, None, 8960, 20224, 20736, 21248, 21504, 22272, 354048, 685824, 713472]
    assert _plan(rows, 64, cap=3) == (3, 55296, [0, 4352, 8704, None, 8960, 20224, 20736, 21248, 21504, 22272, 37888, 53504, 55040])
    # first period only: no room for the pilots
    rows[10] = ("per", 0)
    assert _plan(rows, 64, cap=3) == (3, 39680, [0, 4352, 8704, None, 8960, 20224, 20736, 21248, 21504, 22272, None, 37888, 39424])


def _advance_rows(warm):
    """7 x 54 x 12, K = 1, Mg = 5 (peak, flat and max rows), 12 horizons, 13 arrivals with 20 rate entries, a peak series
    of 18 per problem: q_table h_scal h_row a_seg a_evse a_slot a_len a_cap a_rate_seg a_min a_max | lb ub s_off s_len
    s_cap dfloor applied status x y peak_series | horizon lb ub q pdiag s_off s_len s_cap peak lf dc dfloor warm_x warm_y
    flags"""
    wx, wy = (NV, 5 * 12 * 8) if warm else (0, 0)
    return (whole(12 * NV, 12 * 24, 13 * 4, 8 * 4, 13 * 4, 13 * 4, 13 * 4, 13 * 8, 14 * 4, 20 * 8, 20 * 8)
            + per(NV, NV, 54 * 4, 54 * 4, 54 * 8, 8, 54 * 8, 4, wx, wy, 18 * 8)
            + per(4, NV, NV, NV, 8, 54 * 4, 54 * 4, 54 * 8, 12 * 8, 8, 8, 8, wx, wy, 4))


def test_advance_table_with_and_without_warm_outputs():
    plan_offs = [0, 62208, 62720, 62976, 63232, 63488, 63744, 64000, 64256, 64512, 64768]
    chunk, need, offs = _plan(_advance_rows(True), 7)
    assert (chunk, need) == (7, 345856) and offs[:11] == plan_offs
    assert offs[11:] == [65024, 101376, 137728, 139264, 140800, 143872, 144128, 147200, 147456, 183808, 187392, 188416, 188672, 225024,
                         261376, 297728, 297984, 299520, 301056, 304128, 304896, 305152, 305408, 305664, 342016, 345600]
    chunk, need, offs = _plan(_advance_rows(True), 7, cap=3)
    assert (chunk, need) == (3, 188160) and offs[:12] == plan_offs + [65024] and offs[19:21] == [101376, 116992] and offs[-1] == 187904
    chunk, need, offs = _plan(_advance_rows(False), 7)
    assert (chunk, need) == (7, 265984) and offs[:11] == plan_offs
    assert offs[19:22] == [None, None, 147456] and offs[33:] == [265472, None, None, 265728]   # x, y, warm_x, warm_y: no room
    assert _plan(_advance_rows(False), 7, cap=3)[:2] == (3, 153856)
    assert _plan(_advance_rows(True), 100000)[0] == BUDGET // 39700 == 6761 and _plan(_advance_rows(False), 100000)[0] == BUDGET // 28372 == 9461


# ---- the overlap predicate ------------------------------------------------------------------------------------------------
def test_spans_meet():
    m = _lib().meet
    assert m(1000, 16, 2000, 16) == 0 and m(2000, 16, 1000, 16) == 0          # disjoint
    assert m(1000, 16, 1016, 8) == 0 and m(1016, 8, 1000, 16) == 0            # touching: the end equals the begin
    assert m(1000, 16, 1015, 8) == 1 and m(1015, 8, 1000, 16) == 1            # one byte shared
    assert m(1000, 100, 1010, 5) == 1 and m(1010, 5, 1000, 100) == 1          # containment
    assert m(1000, 16, 1000, 16) == 1
    assert m(0, 16, 1000, 16) == 0 and m(1000, 16, 0, 16) == 0 and m(0, 16, 0, 16) == 0   # a null pointer
    assert m(1000, 0, 1000, 16) == 0 and m(1000, 16, 1004, 0) == 0            # an empty span, even inside the other
