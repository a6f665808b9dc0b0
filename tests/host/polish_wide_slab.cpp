// Stand-alone host check of the wide-site polish's storage (adacharge_amd/csrc/acn_qp_polwide.hpp): for every shape the
// route's predicate admits on a grid of (N, t_max, K, Mg) the slab and the LDS are allocated at exactly the size the layout
// states, carved up as the kernel carves them (acn_qp_polish_wide.hpp), and every table is written from its first to its
// last entry at the worst case of the shape.  Built with -fsanitize=address,undefined by tests/test_polish_wide_host.py: a
// table that overruns the slab, or two that overlap (the fill values are checked afterwards), fail the run.  Also: the
// codes of the ratio test keep the order (kind, p0, p1) up to EVSE 1,023, and the predicate refuses what the tables do not
// hold.  No GPU, no Python inside.  Prints one JSON line with the slab sizes DESIGN.md reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "acn_qp_polwide.hpp"

namespace {

int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; std::fprintf(stderr, "FAILED %s (line %d)\n", #c, __LINE__); } } while (0)

struct Table { long long off_bytes, bytes; };

// fill every table with its own value, then look at each one's first and last byte: an overlap or an overrun shows
void fill_and_check(unsigned char* base, long long total_bytes, const std::vector<Table>& tabs) {
  for (size_t k = 0; k < tabs.size(); ++k) {
    CHECK(tabs[k].off_bytes >= 0 && tabs[k].bytes > 0 && tabs[k].off_bytes + tabs[k].bytes <= total_bytes);
    std::memset(base + tabs[k].off_bytes, (int)(k + 1), (size_t)tabs[k].bytes);
  }
  for (size_t k = 0; k < tabs.size(); ++k)
    CHECK(base[tabs[k].off_bytes] == (unsigned char)(k + 1) && base[tabs[k].off_bytes + tabs[k].bytes - 1] == (unsigned char)(k + 1));
  for (size_t a = 0; a < tabs.size(); ++a)
    for (size_t b = a + 1; b < tabs.size(); ++b)
      CHECK(tabs[a].off_bytes + tabs[a].bytes <= tabs[b].off_bytes || tabs[b].off_bytes + tabs[b].bytes <= tabs[a].off_bytes);
}

void one_shape(int N, int Tm, int K, int Mg, int nrow) {
  using namespace acnqp;
  CHECK(polish_wide_holds(N, Tm, K, Mg, nrow));
  const PolishWideLayout L(N, Tm, K, Mg, nrow);
  CHECK(L.max_rows == Mg * Tm && L.max_sess >= N * K && L.max_sess <= kPolWideMaxSess && L.mt_max == Mg);
  CHECK(L.lds_bytes() <= kPolWideLdsBytes && L.lds_bytes() == L.lds_total * 8);
  const long long nv = (long long)N * Tm, capd = (long long)L.max_sess * (L.max_sess + 1) / 2;
  // ---- the slab, as the kernel carves it -----------------------------------------------------------------------------
  std::vector<double> slab((size_t)L.slab_total);
  std::vector<Table> tabs;
  for (long long o : {L.x, L.d, L.g, L.e, L.lb, L.ub, L.q, L.rn}) tabs.push_back({o * 8, nv * 8});
  for (long long o : {L.u, L.du}) tabs.push_back({o * 8, (long long)Mg * Tm * 8});
  tabs.push_back({L.nu * 8, (long long)nrow * Tm * 8});
  for (long long o : {L.rc0, L.rc1, L.rca, L.rdg, L.lam}) tabs.push_back({o * 8, (long long)L.max_rows * 8});
  tabs.push_back({L.blk * 8, (long long)Tm * L.blk_one * 8});
  tabs.push_back({L.zb * 8, (long long)L.mt_max * N * 8});
  tabs.push_back({L.cap * 8, capd * 8});
  for (long long o : {L.snf, L.sce, L.smu}) tabs.push_back({o * 8, 4LL * N * 8});
  const size_t doubles = tabs.size();
  for (int k = 0; k < 3; ++k) tabs.push_back({L.itab * 8 + (long long)k * L.max_rows * 4, (long long)L.max_rows * 4});   // RJ, RR, RT
  tabs.push_back({L.btab * 8, nv});                                            // ST
  tabs.push_back({L.btab * 8 + nv, nv});                                       // CS
  tabs.push_back({L.btab * 8 + 2 * nv, (long long)nrow * Tm});                 // RACT
  tabs.push_back({L.btab * 8 + 2 * nv + (long long)nrow * Tm, 4LL * N});       // SFL
  fill_and_check(reinterpret_cast<unsigned char*>(slab.data()), L.slab_bytes(), tabs);
  for (size_t k = 0; k < doubles; ++k) CHECK(tabs[k].off_bytes % 8 == 0);
  CHECK(L.slab_total % 2 == 0);
  // ---- LDS -----------------------------------------------------------------------------------------------------------
  std::vector<double> lds((size_t)L.lds_total);
  std::vector<Table> lt;
  lt.push_back({L.wblk * 8LL, 4LL * L.blk_one * 8});
  lt.push_back({L.wvec * 8LL, 4LL * 2 * L.mt_max * 8});
  for (int o : {L.zv, L.sisq, L.di}) lt.push_back({o * 8LL, (long long)L.max_sess * 8});
  lt.push_back({L.red * 8LL, 16 * 8});
  // the int tables in the kernel's order: TSTART, BOFF [Tm + 1]; SI, SKS, S0, S1 [max_sess]; COLOF [4 N]; ACT, ACTI [N]; MISC [8]
  long long io = L.ints * 8LL;
  for (long long n : {(long long)Tm + 1, (long long)Tm + 1, (long long)L.max_sess, (long long)L.max_sess, (long long)L.max_sess,
                      (long long)L.max_sess, 4LL * N, (long long)N, (long long)N, 8LL}) {
    lt.push_back({io, n * 4});
    io += n * 4;
  }
  CHECK(io - L.ints * 8LL == L.nints(N, Tm) * 4);
  fill_and_check(reinterpret_cast<unsigned char*>(lds.data()), L.lds_bytes(), lt);
}

}  // namespace

int main() {
  using namespace acnqp;
  int shapes = 0;
  for (int N : {65, 66, 72, 80, 128, 129, 130, 256, 257, 512, 1023, 1024})
    for (int Tm : {1, 3, 5, 8, 12, 17, 33, 47, 48})
      for (int K : {1, 2, 3, 4})
        for (int Mg : {1, 2, 10, 11, 20, 28, 44, 47, 48}) {
          if (!polish_wide_holds(N, Tm, K, Mg, Mg)) {   // (only the session columns can refuse on this grid)
            CHECK(polish_long_sess(N, K) > kPolWideMaxSess);
            continue;
          }
          const int nrow_soc = (Mg + 1) / 2, nrow_lin = Mg;   // discs (+ a peak row when Mg is odd); box rows
          one_shape(N, Tm, K, Mg, nrow_soc);
          one_shape(N, Tm, K, Mg, nrow_lin);
          shapes += 2;
        }
  CHECK(!polish_wide_holds(64, 12, 1, 16, 8) && !polish_wide_holds(1025, 12, 1, 16, 8) && !polish_wide_holds(80, 49, 1, 16, 8));
  CHECK(!polish_wide_holds(80, 12, 5, 16, 8) && !polish_wide_holds(80, 12, 1, 16, 0) && !polish_wide_holds(80, 12, 1, 49, 8));
  CHECK(!polish_wide_holds(257, 12, 4, 16, 8) && polish_wide_holds(256, 12, 4, 16, 8) && polish_wide_holds(1024, 48, 1, 48, 24));
  // the codes: one order for (kind, p0, p1), round trip, positive
  int prev = -1;
  for (int kind = 0; kind < 4; ++kind)
    for (int p0 = 0; p0 < kPolWideMaxN; ++p0)
      for (int p1 = 0; p1 < kPolWideMaxT; ++p1) {
        const int c = pol_code_long(kind, p0, p1);
        CHECK(c > prev || (kind == 0 && p0 == 0 && p1 == 0));
        CHECK(pol_code_long_kind(c) == kind && pol_code_long_p0(c) == p0 && pol_code_long_p1(c) == p1);
        prev = c;
      }
  const PolishWideLayout a(512, 48, 2, 28, 14), b(1024, 48, 1, 48, 24);
  std::printf("{\"failures\": %d, \"shapes\": %d, \"slab_bytes_512x48\": %lld, \"lds_bytes_512x48\": %d, \"slab_bytes_1024x48\": %lld, "
              "\"lds_bytes_1024x48\": %d}\n",
              failures, shapes, a.slab_bytes(), a.lds_bytes(), b.slab_bytes(), b.lds_bytes());
  return failures ? 1 : 0;
}
