"""The tables of a chunk's arrays and of the session-table staging (Part 1 of adacharge_amd/csrc/acn_qp_pipeline.hpp),
compiled for the host (g++, as tests/test_route_table.py compiles the planner) and checked without a GPU.  The harness
below restates the layout arithmetic as it stood BEFORE there was a table -- one offset line per array -- as a frozen
specification: the table must give exactly those offsets, in the same order, every array on a 256-byte line."""
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
#include "acn_qp_pipeline.hpp"
using namespace acnqp;

// ---- the frozen specification: the layout as it was written out, array by array -----------------------------------------
struct SpecLayout {
  size_t lb, ub, q, pd, hz, so, sl, sc, eq, pk, lf, dc, df, xh, wx, wy, in_total;
  size_t x, st, it, pr, du, ob, y, out_total;
  SpecLayout(size_t cn, size_t N, size_t Tm, size_t K, size_t Mg, bool peak, bool flat, bool mx, bool warm, bool want_y, bool direct) {
    size_t o = 0;
    lb = o; o += al256(cn * N * Tm * 8);
    ub = o; o += al256(cn * N * Tm * 8);
    q = o;  o += al256(cn * N * Tm * 8);
    pd = o; o += al256(cn * 8);
    hz = o; o += al256(cn * 4);
    so = o; o += al256(cn * K * N * 4);
    sl = o; o += al256(cn * K * N * 4);
    sc = o; o += al256(cn * K * N * 8);
    eq = o; o += al256(cn);
    pk = o; o += al256(peak ? cn * Tm * 8 : 0);
    lf = o; o += al256(flat ? cn * 8 : 0);
    dc = o; o += al256(mx ? cn * 8 : 0);
    df = o; o += al256(mx ? cn * 8 : 0);
    xh = o; o += al256(direct ? cn * sizeof(double*) : 0);
    wx = o; o += al256(warm ? cn * N * Tm * 8 : 0);
    wy = o; o += al256(warm ? cn * Mg * Tm * 8 : 0);
    in_total = o;
    o = 0;
    x = o;  o += al256(cn * N * Tm * 8);
    st = o; o += al256(cn * 4);
    it = o; o += al256(cn * 4);
    pr = o; o += al256(cn * 8);
    du = o; o += al256(cn * 8);
    ob = o; o += al256(cn * 8);
    y = o;  o += al256(want_y ? cn * Mg * Tm * 8 : 0);
    out_total = o;
  }
};
struct SpecTable {
  size_t qi, sg, ev, sl, of, ln, rs, cp, mn, mxr, qt, total;
  SpecTable(long long cn, long long ns, long long nr, size_t H, size_t nv) {
    size_t o = 0;
    qi = o; o += al256((size_t)cn * 4);
    sg = o; o += al256((size_t)(cn + 1) * 4);
    ev = o; o += al256((size_t)ns * 4);
    sl = o; o += al256((size_t)ns * 4);
    of = o; o += al256((size_t)ns * 4);
    ln = o; o += al256((size_t)ns * 4);
    rs = o; o += al256((size_t)(ns + 1) * 4);
    cp = o; o += al256((size_t)ns * 8);
    mn = o; o += al256((size_t)nr * 8);
    mxr = o; o += al256((size_t)nr * 8);
    qt = o; o += al256(H * nv * 8);
    total = o;
  }
};

// one side of a layout against the rules every row obeys; fails[1..3] count the violations
static void check_side(const ArrayRow* rows, int n, const size_t* off, size_t total, const ChunkShape& s, size_t lo, size_t bytes, long long* fails) {
  size_t small_sum = 0;
  for (int k = 0; k < n; ++k) {
    const size_t len = (k + 1 < n ? off[k + 1] : total) - off[k];
    const bool here = present(rows[k], s);
    if (here && off[k] % 256 != 0) ++fails[1];                         // a present array: on a 256-byte line
    if (!here && len != 0) ++fails[2];                                 // an absent array: no bytes
    const bool inside = off[k] >= lo && off[k] + len <= lo + bytes;
    if (rows[k].size == Size::Small) { small_sum += len; if (!inside) ++fails[3]; }   // the mirror range holds every small row,
    else if (len != 0 && off[k] < lo + bytes && off[k] + len > lo) ++fails[3];        // no byte of a large row,
  }
  if (small_sum != bytes) ++fails[3];                                                 // and nothing else
}

extern "C" {
// the sweep of the issue: every offset and both totals against the specification; fails[0] counts layouts that differ,
// fails[4] the layouts seen
void sweep(long long* fails) {
  const size_t cns[] = {1, 7, 256, 8192}, Ns[] = {1, 54, 512}, Tms[] = {1, 12, 48, 144}, Ks[] = {1, 2, 4}, Mgs[] = {0, 5, 48};
  for (size_t cn : cns) for (size_t N : Ns) for (size_t Tm : Tms) for (size_t K : Ks) for (size_t Mg : Mgs)
    for (int m = 0; m < 64; ++m) {
      const bool peak = m & 1, flat = m & 2, mx = m & 4, warm = m & 8, want_y = m & 16, direct = m & 32;
      const SpecLayout S(cn, N, Tm, K, Mg, peak, flat, mx, warm, want_y, direct);
      const ChunkShape shape{N, Tm, K, Mg, peak, flat, mx, warm, want_y, direct};
      const ChunkLayout L(cn, shape);
      const size_t in[] = {S.lb, S.ub, S.q, S.pd, S.hz, S.so, S.sl, S.sc, S.eq, S.pk, S.lf, S.dc, S.df, S.xh, S.wx, S.wy};
      const size_t out[] = {S.x, S.st, S.it, S.pr, S.du, S.ob, S.y};
      static_assert(sizeof(in) / sizeof(in[0]) == kInRows && sizeof(out) / sizeof(out[0]) == kOutRows, "16 input and 7 result arrays");
      bool same = L.in[kInRows] == S.in_total && L.out[kOutRows] == S.out_total && L.cn == cn && L.direct == direct;
      for (int k = 0; k < kInRows; ++k) same = same && L.in[k] == in[k];
      for (int k = 0; k < kOutRows; ++k) same = same && L.out[k] == out[k];
      // the mirrors: what used to be written [pd, wx) and [st, y)
      same = same && L.mirror_in() == S.pd && L.mirror_in_bytes() == S.wx - S.pd && L.mirror_out() == S.st && L.mirror_out_bytes() == S.y - S.st;
      if (!same) ++fails[0];
      check_side(kIn, kInRows, L.in, L.in[kInRows], shape, L.mirror_in(), L.mirror_in_bytes(), fails);
      check_side(kOut, kOutRows, L.out, L.out[kOutRows], shape, L.mirror_out(), L.mirror_out_bytes(), fails);
      ++fails[4];
    }
}
// one layout, for the values written out in the test: in[16], in_total, out[7], out_total
void layout(long long cn, long long N, long long Tm, long long K, long long Mg, int m, long long* o) {
  const ChunkLayout L((size_t)cn, ChunkShape{(size_t)N, (size_t)Tm, (size_t)K, (size_t)Mg, (m & 1) != 0, (m & 2) != 0, (m & 4) != 0, (m & 8) != 0, (m & 16) != 0, (m & 32) != 0});
  for (int k = 0; k <= kInRows; ++k) *o++ = (long long)L.in[k];     // (the last one: the side's bytes)
  for (int k = 0; k <= kOutRows; ++k) *o++ = (long long)L.out[k];
}
// the table staging against its specification: 1 if every offset and the total are equal; o: off[11], total
int table_layout(long long lo, long long cn, long long s0, long long ns, long long r0, long long nr, long long H, long long nv, long long* o) {
  TableSpan sp;
  sp.lo = lo; sp.cn = cn; sp.s0 = s0; sp.ns = ns; sp.r0 = r0; sp.nr = nr; sp.qt = (size_t)(H * nv);
  const TableLayout TL(sp);
  const SpecTable S(cn, ns, nr, (size_t)H, (size_t)nv);
  const size_t spec[] = {S.qi, S.sg, S.ev, S.sl, S.of, S.ln, S.rs, S.cp, S.mn, S.mxr, S.qt};
  static_assert(sizeof(spec) / sizeof(spec[0]) == kTableRows, "11 staged arrays");
  bool same = TL.total == S.total;
  for (int k = 0; k < kTableRows; ++k) { same = same && TL.off[k] == spec[k]; o[k] = (long long)TL.off[k]; }
  o[kTableRows] = (long long)TL.total;
  return same;
}
// row k of the table staging: first element and element count of the source array for the span
void table_row(int k, long long lo, long long cn, long long s0, long long ns, long long r0, long long nr, long long qt, long long* o) {
  TableSpan sp;
  sp.lo = lo; sp.cn = cn; sp.s0 = s0; sp.ns = ns; sp.r0 = r0; sp.nr = nr; sp.qt = (size_t)qt;
  o[0] = (long long)table_base(kTable[k], sp); o[1] = (long long)table_count(kTable[k], sp); o[2] = kTable[k].elem;
  o[3] = (long long)kTable[k].field; o[4] = (long long)kTable[k].arg;
}

// coverage.  The pointer members of a struct are its words from `first` on (sizeof / offsetof, never a count written
// here): rows[w] = how many rows of the table name word w, -1 for a row that names no word of the struct
static int count_rows(const ArrayRow* rows, int n, size_t first, size_t size, int* per_word) {
  const int words = (int)((size - first) / sizeof(void*));
  for (int w = 0; w < words; ++w) per_word[w] = 0;
  int none = 0;
  for (int k = 0; k < n; ++k) {
    if (rows[k].field == kNoField) { ++none; continue; }
    if (rows[k].field < first || rows[k].field >= size || (rows[k].field - first) % sizeof(void*) != 0) return -1;
    ++per_word[(rows[k].field - first) / sizeof(void*)];
  }
  return none;
}
int in_words() { return (int)((sizeof(acnqp_problems) - offsetof(acnqp_problems, horizon)) / sizeof(void*)); }
int out_words() { return (int)(sizeof(acnqp_results) / sizeof(void*)); }
int x_dev_word() { return (int)(offsetof(acnqp_results, x_dev) / sizeof(void*)); }
int in_coverage(int* per_word) { return count_rows(kIn, kInRows, offsetof(acnqp_problems, horizon), sizeof(acnqp_problems), per_word); }
int out_coverage(int* per_word) { return count_rows(kOut, kOutRows, 0, sizeof(acnqp_results), per_word); }
// the names: row `k` of the enum is the array of that name
int names_hold() {
#define IN(k, f) (kIn[k].field == offsetof(acnqp_problems, f))
#define OUT(k, f) (kOut[k].field == offsetof(acnqp_results, f))
  return IN(kLb, lb) && IN(kUb, ub) && IN(kQ, q) && IN(kPd, pdiag) && IN(kHz, horizon) && IN(kSo, s_off) && IN(kSl, s_len) && IN(kSc, s_cap) &&
         IN(kEq, s_eq) && IN(kPk, peak) && IN(kLf, lf) && IN(kDc, dc) && IN(kDf, dfloor) && kIn[kXh].field == kNoField && IN(kWx, warm_x) &&
         IN(kWy, warm_y) && OUT(kX, x) && OUT(kSt, status) && OUT(kIt, iters) && OUT(kPr, pri_res) && OUT(kDu, dua_res) && OUT(kOb, obj) && OUT(kY, y);
}
int small_range(int side, int* r) {
  const RowRange g = side == 0 ? kSmallIn : kSmallOut;
  r[0] = g.first; r[1] = g.end;
  return side == 0 ? (int)kInRows : (int)kOutRows;
}
}
"""


@functools.lru_cache(maxsize=None)
def _lib():
    tmp = tempfile.mkdtemp(prefix="acnqp_layout_")
    src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.run([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-I" + INC, src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    shutil.rmtree(tmp)   # (the mapping stays; nothing built is left behind)
    LL, I, P = ctypes.c_longlong, ctypes.c_int, ctypes.POINTER
    lib.sweep.restype, lib.sweep.argtypes = None, [P(LL)]
    lib.layout.restype, lib.layout.argtypes = None, [LL] * 5 + [I, P(LL)]
    lib.table_layout.restype, lib.table_layout.argtypes = I, [LL] * 8 + [P(LL)]
    lib.table_row.restype, lib.table_row.argtypes = None, [I] + [LL] * 7 + [P(LL)]
    for name in ("in_coverage", "out_coverage"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = I, [P(I)]
    lib.small_range.restype, lib.small_range.argtypes = I, [I, P(I)]
    return lib


PEAK, FLAT, MAX, WARM, WANT_Y, DIRECT = 1, 2, 4, 8, 16, 32


def _layout(cn, N, Tm, K, Mg, flags):
    out = (ctypes.c_longlong * 25)()
    _lib().layout(cn, N, Tm, K, Mg, flags, out)
    v = [int(x) for x in out]
    return v[:16], v[16], v[17:24], v[24]


# ---- a chunk's arrays -------------------------------------------------------------------------------------------------------
def test_every_offset_equals_the_written_out_layout_over_the_sweep():
    """cn 1, 7, 256, 8192 x N 1, 54, 512 x Tm 1, 12, 48, 144 x K 1, 2, 4 x Mg 0, 5, 48 x the 64 combinations of peak, flat,
    max, warm, want_y, direct"""
    fails = (ctypes.c_longlong * 5)()
    _lib().sweep(fails)
    assert fails[4] == 4 * 3 * 4 * 3 * 3 * 64 == 27648
    assert fails[0] == 0, "offsets, totals or mirror ranges differ from the specification"
    assert fails[1] == 0, "a present array does not start on a 256-byte line"
    assert fails[2] == 0, "an absent array takes bytes"
    assert fails[3] == 0, "the small rows of a side are not one range free of large rows"


def test_one_layout_written_out():
    """7 problems of 54 x 12, K = 2, Mg = 5, every optional array: lb ub q pd hz so sl sc eq pk lf dc df xh wx wy | x st it
    pr du ob y"""
    nv = 7 * 54 * 12 * 8   # 36,288 -> 36,352
    assert -(-nv // 256) * 256 == 36352
    ins, in_total, outs, out_total = _layout(7, 54, 12, 2, 5, PEAK | FLAT | MAX | WARM | WANT_Y | DIRECT)
    assert ins == [0, 36352, 72704, 109056, 109312, 109568, 112640, 115712, 121856, 122112, 122880, 123136, 123392, 123648, 123904, 160256]
    assert in_total == 160256 + 3584          # warm_y: 7 x 5 x 12 x 8 = 3,360 -> 3,584
    assert outs == [0, 36352, 36608, 36864, 37120, 37376, 37632] and out_total == 37632 + 3584
    # nothing optional: the absent arrays sit on their neighbour's offset and add nothing
    ins, in_total, outs, out_total = _layout(7, 54, 12, 2, 5, 0)
    assert ins[9:] == [122112] * 7 and in_total == 122112 and outs[6] == out_total == 37632


def test_small_rows_stand_together():
    r = (ctypes.c_int * 2)()
    assert _lib().small_range(0, r) == 16 and list(r) == [3, 14]   # pd ... xh
    assert _lib().small_range(1, r) == 7 and list(r) == [1, 6]     # st ... ob


def test_every_pointer_of_the_abi_structs_has_exactly_one_row():
    lib = _lib()
    n_in, n_out = lib.in_words(), lib.out_words()
    assert n_in >= 15 and n_out >= 8          # (what include/acn_qp.h holds today; a member added later raises these by itself)
    per = (ctypes.c_int * n_in)()
    assert lib.in_coverage(per) == 1          # one row without a member: xh
    assert list(per) == [1] * n_in
    per = (ctypes.c_int * n_out)()
    assert lib.out_coverage(per) == 0
    expect = [1] * n_out
    expect[lib.x_dev_word()] = 0              # a destination of x, not an array of the chunk
    assert list(per) == expect
    assert lib.names_hold() == 1


# ---- the session-table staging ------------------------------------------------------------------------------------------
def test_table_staging_equals_the_written_out_layout():
    out = (ctypes.c_longlong * 12)()
    for lo, cn, s0, ns, r0, nr, H, nv in [(0, 1, 0, 0, 0, 0, 1, 1), (0, 96, 0, 1500, 0, 9000, 12, 54 * 12), (40, 24, 611, 377, 3000, 2262, 12, 54 * 12),
                                          (8191, 8192, 10 ** 6, 130000, 10 ** 7, 800000, 48, 512 * 48), (5, 7, 3, 0, 9, 0, 144, 54 * 144),
                                          (0, 63, 0, 64, 0, 31, 1, 7)]:
        assert _lib().table_layout(lo, cn, s0, ns, r0, nr, H, nv, out) == 1, (cn, ns, nr, H, nv)
        assert all(o % 256 == 0 for o in out)
    # one written out: 24 problems, 377 sessions, 2,262 rate entries, 12 horizons of 54 x 12
    assert _lib().table_layout(40, 24, 611, 377, 3000, 2262, 12, 648, out) == 1
    assert list(out) == [0, 256, 512, 2048, 3584, 5120, 6656, 8192, 11264, 29440, 47616, 47616 + 62208]
    # no sessions: their arrays take no bytes, rate_seg keeps its one entry
    assert _lib().table_layout(5, 7, 3, 0, 9, 0, 1, 1, out) == 1
    assert list(out) == [0, 256, 512, 512, 512, 512, 512, 768, 768, 768, 768, 1024]


def test_table_rows_start_and_count():
    """q_index sess_seg s_evse s_slot s_off s_len rate_seg s_cap min_rates max_rates q_table: (first element, elements,
    element size) for the chunk of problems [40, 64) with sessions [611, 988) and rate entries [3000, 5262)"""
    got = []
    o = (ctypes.c_longlong * 5)()
    for k in range(11):
        _lib().table_row(k, 40, 24, 611, 377, 3000, 2262, 7776, o)
        got.append((int(o[0]), int(o[1]), int(o[2])))
    assert got == [(40, 24, 4), (40, 25, 4), (611, 377, 4), (611, 377, 4), (611, 377, 4), (611, 377, 4), (611, 378, 4), (611, 377, 8),
                   (3000, 2262, 8), (3000, 2262, 8), (0, 7776, 8)]
