// Storage of the long-horizon polish (acn_qp_polish_long.hpp): what a workgroup keeps in its slab of global memory and
// what it keeps in LDS, as offsets computed ONCE from the shape -- the host sizes the slab and the LDS from this struct
// and the kernel carves both up with it.  Every table is sized for the worst case of the shape: every site row tight in
// every period with its tangent row (Mg rows per period: two per disc, one per box or peak row), every session slot a
// column of V.  So no problem of such a shape is ever declined or given up for `rows`.
// Host-compilable: tests/host/polish_long_slab.cpp checks the carve-up under a sanitizer.
#pragma once
#include <stdint.h>

#include <algorithm>

#if defined(__HIPCC__)
#define ACNQP_SLAB_FN __host__ __device__ inline
#else
#define ACNQP_SLAB_FN inline
#endif

namespace acnqp {

constexpr int kPolLongMinT = 33;         // horizons the long polish serves: the first beyond polish_kernel<8> ...
constexpr int kPolLongMaxT = 288;        // ... to the offline day
constexpr int kPolLongMaxN = 64;         // EVSEs: a quad of threads each
constexpr int kPolLongMaxSess = 256;     // session columns at most: one thread per column in the capacitance solves
constexpr int kPolLongGrid = 32;         // workgroups (slabs) of a launch at most: the list is short
constexpr int kPolLongLdsBytes = 152 * 1024;   // LDS a workgroup may take (one per CU)
constexpr int kPolLongActive = 64;       // session columns that touch ONE period at most: one per EVSE (windows of an EVSE are disjoint)

// blocking-constraint / release codes of the long polish: kind in the top bits, 16 bits for an EVSE or site row, 12 for a
// period or session slot (pol_code of acn_qp_polish.hpp gives a period 8).  Ordered like (kind, p0, p1): ties go to the
// smaller code.
ACNQP_SLAB_FN int pol_code_long(int kind, int p0, int p1) { return (kind << 28) | (p0 << 12) | p1; }
ACNQP_SLAB_FN int pol_code_long_kind(int code) { return code >> 28; }
ACNQP_SLAB_FN int pol_code_long_p0(int code) { return (code >> 12) & 0xffff; }
ACNQP_SLAB_FN int pol_code_long_p1(int code) { return code & 0xfff; }

// rows of the Schur system at most, session columns at most (a multiple of 8), rows of one period's block at most
ACNQP_SLAB_FN int polish_long_rows(int Mg, int Tm) { return Mg * Tm; }
ACNQP_SLAB_FN int polish_long_sess(int N, int K) { return ((N * K + 7) / 8) * 8; }

struct PolishLongLayout {
  int max_rows, max_sess, mt_max, blk_one;   // blk_one: doubles of one period's packed block at most
  bool cap_in_lds;                           // the capacitance matrix fits the LDS budget (else: in the slab)
  // ---- slab, offsets in doubles --------------------------------------------------------------------------------------
  long long x, d, g, e, lb, ub, q, rn;       // (N, Tm): iterate, step (first: v_free, R' lam), gradient, e, bounds, q, normal rows' R' lam
  long long u, du;                           // (Mg, Tm): G x, G dx
  long long nu;                              // (nrow, Tm): multipliers of the site rows
  long long rc0, rc1, rca, rdg, lam;         // [max_rows]: the Schur rows' coefficients, residual, diagonal / 1 / D, multiplier
  long long blk;                             // Tm blocks, packed lower, one after the other
  long long cap;                             // capacitance matrix, packed lower (cap_in_lds: nothing)
  long long itab;                            // ints: RJ, RR, RT [max_rows] each, one after the other
  long long btab;                            // bytes: (N, Tm) bound status, (N, Tm) session column of a free variable, (nrow, Tm) tight rows
  long long slab_total;
  // ---- LDS, offsets in doubles ---------------------------------------------------------------------------------------
  int gs, wblk, wvec, zb, zv, sisq, di, red, lcap, ints, lds_total;

  ACNQP_SLAB_FN PolishLongLayout(int N, int Tm, int K, int Mg, int nrow) {
    max_rows = polish_long_rows(Mg, Tm);
    max_sess = polish_long_sess(N, K);
    mt_max = Mg;
    blk_one = mt_max * (mt_max + 1) / 2;
    const long long nv = (long long)N * Tm, cap_doubles = (long long)max_sess * (max_sess + 1) / 2;
    // LDS first: it decides where the capacitance matrix lives
    int l = 0;
    gs = l; l += Mg * N;
    wblk = l; l += 4 * blk_one;                      // the block in work of each wave
    wvec = l; l += 4 * 2 * mt_max;                   // ... its right-hand side and 1 / D
    zb = l; l += mt_max * kPolLongActive;            // L_t^-1 V_t of the block in work
    zv = l; l += max_sess;
    sisq = l; l += max_sess;
    di = l; l += max_sess;
    red = l; l += 16;
    ints = l;   // TSTART, BOFF [Tm + 1]; SI, SKS, S0, S1 [max_sess]; COLOF [4 N]; ACT, ACTI [kPolLongActive]; MISC [8]
    const int nint = 2 * (Tm + 1) + 4 * max_sess + 4 * N + 2 * kPolLongActive + 8;
    l += (nint + 1) / 2;
    cap_in_lds = ((long long)l + cap_doubles) * 8 <= kPolLongLdsBytes;
    lcap = l; l += cap_in_lds ? (int)cap_doubles : 0;
    lds_total = l;
    long long o = 0;
    x = o; o += nv;
    d = o; o += nv;
    g = o; o += nv;
    e = o; o += nv;
    lb = o; o += nv;
    ub = o; o += nv;
    q = o; o += nv;
    rn = o; o += nv;
    u = o; o += (long long)Mg * Tm;
    du = o; o += (long long)Mg * Tm;
    nu = o; o += (long long)nrow * Tm;
    rc0 = o; o += max_rows;
    rc1 = o; o += max_rows;
    rca = o; o += max_rows;
    rdg = o; o += max_rows;
    lam = o; o += max_rows;
    blk = o; o += (long long)Tm * blk_one;
    cap = o; o += cap_in_lds ? 0 : cap_doubles;
    itab = o; o += (3LL * max_rows + 1) / 2;
    btab = o; o += (2 * nv + (long long)nrow * Tm + 7) / 8;
    slab_total = (o + 1) & ~1LL;                     // (16-byte multiple per workgroup)
  }
  ACNQP_SLAB_FN long long slab_bytes() const { return slab_total * 8; }
  ACNQP_SLAB_FN int lds_bytes() const { return lds_total * 8; }
};

// doubles of ONE workgroup's slab for a shape (the launch reserves this times its grid)
ACNQP_SLAB_FN long long polish_long_slab_doubles(int N, int Tm, int K, int Mg, int nrow) {
  return PolishLongLayout(N, Tm, K, Mg, nrow).slab_total;
}
// the shapes the kernel's thread map and tables hold (the route's polish_long_shape asks for the same and for the family)
ACNQP_SLAB_FN bool polish_long_holds(int N, int Tm, int K, int Mg, int nrow) {
  return N >= 1 && N <= kPolLongMaxN && Tm >= kPolLongMinT && Tm <= kPolLongMaxT && K >= 1 && N * K <= kPolLongMaxSess &&
         nrow >= 1 && Mg >= nrow && Mg <= 48;
}
// host: workgroups (slabs) of a launch, bytes of the slabs of `grid` workgroups, doubles of the packed per-period blocks
// (PolishArgs.blk_doubles)
inline int polish_long_grid(int batch) { return std::max(1, std::min(batch, kPolLongGrid)); }
inline long long polish_long_slab_bytes(int N, int Tm, int K, int Mg, int nrow, int grid) {
  return PolishLongLayout(N, Tm, K, Mg, nrow).slab_bytes() * std::max(1, std::min(grid, kPolLongGrid));
}
inline int polish_long_block_doubles(int Tm, int Mg) { return Tm * (Mg * (Mg + 1) / 2); }

}  // namespace acnqp
