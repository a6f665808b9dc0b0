// Storage of the on-chip polish (acn_qp_polish.hpp: N <= 64, horizons <= 32): what a workgroup keeps in LDS, as offsets
// computed ONCE from the shape -- the host sizes the LDS from this struct and the kernel carves it up with it -- and the
// sizes of its tables.  Host-compilable, like the long and wide kernels' layouts (acn_qp_polslab.hpp, acn_qp_polwide.hpp):
// the polish plan (acn_qp_polplan.hpp) asks it, and tests/test_polish_plan.py holds it to tests/polish_cases.polish_tables.
#pragma once
#include <algorithm>

#include "acn_qp_polslab.hpp"

namespace acnqp {

// LDS one workgroup may use: the whole CU when alone, half of it when two share the CU
constexpr int kLdsPerCu = 160 * 1024;

constexpr int kPolThreads = 256;      // threads of a workgroup of every polish kernel
constexpr int kPolMaxRows = 256;      // rows of the Schur system at most (row tables; one thread per row in the triangular solves)
constexpr int kPolMaxSess = 128;      // tight sessions with free variables (columns of V) at most (PolishArgs.max_sess <= this)

// LDS carve-up in doubles (host: size; device: offsets)
struct PolishLds {
  int xs, ds, gs, u, du, nu, invn, rc0, rc1, rca, rdg, lam, blk, cap, zb, zv, sisq, red, ints, total;
  int mt_max;   // rows of one period's block at most: two per site row
  ACNQP_SLAB_FN PolishLds(int N, int Tm, int Mg, int nrow, int max_rows, int blk_doubles, int max_sess) {
    int o = 0;
    mt_max = 2 * nrow;
    xs = o; o += N * Tm;
    ds = o; o += N * Tm;
    gs = o; o += Mg * N;
    u = o; o += Mg * Tm;
    du = o; o += Mg * Tm;
    nu = o; o += nrow * Tm;
    invn = o; o += N * 4;
    rc0 = o; o += max_rows;
    rc1 = o; o += max_rows;
    rca = o; o += max_rows;
    rdg = o; o += max_rows;
    lam = o; o += max_rows;
    blk = o; o += blk_doubles;                               // the per-period blocks of B, packed lower, one after the other
    cap = o; o += max_sess * (max_sess + 1) / 2;             // C = I - V' B^-1 V, packed lower
    zb = o; o += mt_max * max_sess;                          // L_t^-1 V_t of the block in work
    zv = o; o += max_sess;                                   // V' y, then w
    sisq = o; o += max_sess;                                 // 1 / sqrt(n_s) of the session columns
    red = o; o += 16;
    ints = o;   // ints from here: rj, rr, rt [max_rows], tstart[Tm + 1], boff[Tm + 1], ract[nrow], misc[8], si / sks [max_sess]; then cs[N * Tm] bytes
    const int nint = 3 * max_rows + 2 * (Tm + 1) + nrow + 8 + 2 * max_sess;
    o += (nint + 1) / 2 + (N * Tm + 7) / 8;
    total = o;
  }
  // doubles for the blocks that fit `bytes` of LDS, at most what the worst case needs (every site row tight in every period)
  static int blocks_that_fit(int N, int Tm, int Mg, int nrow, int max_rows, int max_sess, int bytes) {
    const int worst = Tm * (2 * nrow) * (2 * nrow + 1) / 2;
    const long long fixed = (long long)PolishLds(N, Tm, Mg, nrow, max_rows, 0, max_sess).total * 8;
    const long long room = ((long long)bytes - fixed) / 8;
    return (int)(room < 0 ? 0 : (room < worst ? room : worst));
  }
};

// rows the row tables hold, session columns the capacitance matrix holds, LDS doubles for the per-period blocks (<= the
// worst case; never more than the CU's LDS less 2 KB)
inline int polish_max_rows(int nrow, int Tm) { return std::min(kPolMaxRows, ((2 * nrow * Tm + 7) / 8) * 8); }
inline int polish_max_sess(int N, int K) { return std::min(kPolMaxSess, ((N * K + 7) / 8) * 8); }
inline int polish_blocks_that_fit(int N, int Tm, int Mg, int nrow, int max_sess, int lds_bytes) {
  return PolishLds::blocks_that_fit(N, Tm, Mg, nrow, polish_max_rows(nrow, Tm), max_sess, std::min(lds_bytes, kLdsPerCu - 2048));
}

}  // namespace acnqp
