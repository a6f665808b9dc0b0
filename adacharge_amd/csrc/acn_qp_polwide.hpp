// Storage of the wide-site polish (acn_qp_polish_wide.hpp: 64 < N <= 1,024, horizons <= 48): what a workgroup keeps in
// its slab of global memory and what it keeps in LDS, as offsets computed ONCE from the shape -- the host sizes the slab
// and the LDS from this struct and the kernel carves both up with it, as PolishLongLayout (acn_qp_polslab.hpp) does for
// the long horizons.  Every table is sized for the worst case of the shape: Mg rows per period, every session slot a
// column of V.  So no problem of such a shape is ever given up for `rows`.
//
// Four things the long kernel's layout assumes do NOT hold on a wide site, and the layout says where each went:
//   - G (Mg x N, up to 393 KB) does not fit in LDS: there is no copy of it here at all, the kernel reads the handle's
//     acnqp_site.G from global memory (L2-resident: one array for every workgroup of the launch);
//   - up to N session columns touch ONE period, not 64: L_t^-1 V_t of the period in work is Mg x N and lives in the slab
//     (`zb`, row stride N), and the lists of the columns that touch the period (`act`, `acti`: N ints each) are sized by N;
//   - the capacitance matrix has up to 1,024 columns (524,800 packed doubles): always in the slab (`cap`); its L D L' and
//     its solves loop over columns, no thread owns one;
//   - EVSEs come in tiles of 64 (a quad of threads each, as in the long kernel): what a quad keeps of its EVSE's sessions
//     between phases -- tight?, column?, free variables, residual, multiplier -- lives in the slab per (EVSE, slot)
//     (`snf`, `sce`, `smu`, and the flag bytes behind the (N, Tm) byte tables) and is reloaded per tile.
// Host-compilable: tests/host/polish_wide_slab.cpp checks the carve-up under a sanitizer.
#pragma once
#include <stdint.h>

#include "acn_qp_polslab.hpp"

namespace acnqp {

constexpr int kPolWideMinN = 65;          // EVSEs the wide polish serves: the first beyond the other two polish kernels ...
constexpr int kPolWideMaxN = 1024;        // ... to the large-site kernel's limit
constexpr int kPolWideMaxT = 48;          // horizons of the large-site kernel
constexpr int kPolWideMaxK = 4;           // session slots per EVSE
constexpr int kPolWideMaxSess = 1024;     // session columns at most
constexpr int kPolWideMaxMg = 48;         // rows of acnqp_site.G at most
constexpr int kPolWideGrid = 16;          // workgroups (slabs) of a launch at most: the list is short
constexpr int kPolWideLdsBytes = 152 * 1024;   // LDS a workgroup may take (one per CU)

struct PolishWideLayout {
  int max_rows, max_sess, mt_max, blk_one;   // blk_one: doubles of one period's packed block at most
  // ---- slab, offsets in doubles --------------------------------------------------------------------------------------
  long long x, d, g, e, lb, ub, q, rn;       // (N, Tm): iterate, step (first: v_free, R' lam), gradient, e, bounds, q, normal rows' R' lam
  long long u, du;                           // (Mg, Tm): G x, G dx
  long long nu;                              // (nrow, Tm): multipliers of the site rows
  long long rc0, rc1, rca, rdg, lam;         // [max_rows]: the Schur rows' coefficients, residual, diagonal / 1 / D, multiplier
  long long blk;                             // Tm blocks, packed lower, one after the other
  long long zb;                              // (Mg, N): L_t^-1 V_t of the period in work, a row per Schur row of the block
  long long cap;                             // capacitance matrix, packed lower
  long long snf, sce, smu;                   // (N, 4): a session's free variables, residual cap - sum x, multiplier
  long long itab;                            // ints: RJ, RR, RT [max_rows] each, one after the other
  long long btab;                            // bytes: (N, Tm) bound status, (N, Tm) session column of a free variable, (nrow, Tm) tight rows,
                                             // (N, 4) session flags
  long long slab_total;
  // ---- LDS, offsets in doubles ---------------------------------------------------------------------------------------
  int wblk, wvec, zv, sisq, di, red, ints, lds_total;

  ACNQP_SLAB_FN PolishWideLayout(int N, int Tm, int K, int Mg, int nrow) {
    max_rows = polish_long_rows(Mg, Tm);
    max_sess = polish_long_sess(N, K);
    mt_max = Mg;
    blk_one = mt_max * (mt_max + 1) / 2;
    const long long nv = (long long)N * Tm, cap_doubles = (long long)max_sess * (max_sess + 1) / 2;
    int l = 0;
    wblk = l; l += 4 * blk_one;                      // the block in work of each wave
    wvec = l; l += 4 * 2 * mt_max;                   // ... its right-hand side and 1 / D
    zv = l; l += max_sess;
    sisq = l; l += max_sess;
    di = l; l += max_sess;
    red = l; l += 16;
    ints = l;   // TSTART, BOFF [Tm + 1]; SI, SKS, S0, S1 [max_sess]; COLOF [4 N]; ACT, ACTI [N]; MISC [8]
    l += (int)((nints(N, Tm) + 1) / 2);
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
    zb = o; o += (long long)mt_max * N;
    cap = o; o += cap_doubles;
    snf = o; o += 4LL * N;
    sce = o; o += 4LL * N;
    smu = o; o += 4LL * N;
    itab = o; o += (3LL * max_rows + 1) / 2;
    btab = o; o += (2 * nv + (long long)nrow * Tm + 4LL * N + 7) / 8;
    slab_total = (o + 1) & ~1LL;                     // (16-byte multiple per workgroup)
  }
  ACNQP_SLAB_FN long long nints(int N, int Tm) const { return 2LL * (Tm + 1) + 4LL * max_sess + 4LL * N + 2LL * N + 8; }
  ACNQP_SLAB_FN long long slab_bytes() const { return slab_total * 8; }
  ACNQP_SLAB_FN int lds_bytes() const { return lds_total * 8; }
};

// the shapes the kernel's thread map and tables hold (the route's polish_wide_shape asks for the same and for the family)
ACNQP_SLAB_FN bool polish_wide_holds(int N, int Tm, int K, int Mg, int nrow) {
  return N >= kPolWideMinN && N <= kPolWideMaxN && Tm >= 1 && Tm <= kPolWideMaxT && K >= 1 && K <= kPolWideMaxK &&
         polish_long_sess(N, K) <= kPolWideMaxSess && nrow >= 1 && Mg >= nrow && Mg <= kPolWideMaxMg;
}
// host: workgroups (slabs) of a launch, bytes of the slabs of `grid` workgroups, doubles of the packed per-period blocks
// (PolishArgs.blk_doubles)
inline int polish_wide_grid(int batch) { return std::max(1, std::min(batch, kPolWideGrid)); }
inline long long polish_wide_slab_bytes(int N, int Tm, int K, int Mg, int nrow, int grid) {
  return PolishWideLayout(N, Tm, K, Mg, nrow).slab_bytes() * polish_wide_grid(grid);
}
inline int polish_wide_block_doubles(int Tm, int Mg) { return Tm * (Mg * (Mg + 1) / 2); }

}  // namespace acnqp
