// Stand-alone host check of the long-horizon polish's storage (adacharge_amd/csrc/acn_qp_polslab.hpp): for every shape of a
// sweep the slab and the LDS are allocated at exactly the size the layout states, carved up as the kernel carves them, and
// every table is written from its first to its last entry at the worst case of the shape.  Built with
// -fsanitize=address,undefined by tests/test_polish_long_host.py: a table that overruns the slab, or two that overlap (the
// fill values are checked afterwards), fail the run.  Also: the codes of the ratio test keep the order (kind, p0, p1) up to
// period 287.  No GPU, no Python inside.  Prints one JSON line with the slab sizes DESIGN.md reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "acn_qp_polslab.hpp"

namespace {

int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; std::fprintf(stderr, "FAILED %s (line %d)\n", #c, __LINE__); } } while (0)

struct Table { long long off_bytes, bytes; };

void one_shape(int N, int Tm, int K, int Mg, int nrow) {
  using namespace acnqp;
  CHECK(polish_long_holds(N, Tm, K, Mg, nrow));
  const PolishLongLayout L(N, Tm, K, Mg, nrow);
  CHECK(L.max_rows == Mg * Tm && L.max_sess >= N * K && L.max_sess <= kPolLongMaxSess && L.mt_max == Mg);
  CHECK(L.lds_bytes() <= kPolLongLdsBytes && L.lds_bytes() == L.lds_total * 8);
  const long long nv = (long long)N * Tm, capd = (long long)L.max_sess * (L.max_sess + 1) / 2;
  // ---- the slab, as the kernel carves it -----------------------------------------------------------------------------
  std::vector<double> slab((size_t)L.slab_total);
  unsigned char* base = reinterpret_cast<unsigned char*>(slab.data());
  std::vector<Table> tabs;
  for (long long o : {L.x, L.d, L.g, L.e, L.lb, L.ub, L.q, L.rn}) tabs.push_back({o * 8, nv * 8});
  for (long long o : {L.u, L.du}) tabs.push_back({o * 8, (long long)Mg * Tm * 8});
  tabs.push_back({L.nu * 8, (long long)nrow * Tm * 8});
  for (long long o : {L.rc0, L.rc1, L.rca, L.rdg, L.lam}) tabs.push_back({o * 8, (long long)L.max_rows * 8});
  tabs.push_back({L.blk * 8, (long long)Tm * L.blk_one * 8});
  if (!L.cap_in_lds) tabs.push_back({L.cap * 8, capd * 8});
  for (int k = 0; k < 3; ++k) tabs.push_back({L.itab * 8 + (long long)k * L.max_rows * 4, (long long)L.max_rows * 4});   // RJ, RR, RT
  tabs.push_back({L.btab * 8, nv});                      // ST
  tabs.push_back({L.btab * 8 + nv, nv});                 // CS
  tabs.push_back({L.btab * 8 + 2 * nv, (long long)nrow * Tm});   // RACT
  for (size_t k = 0; k < tabs.size(); ++k) std::memset(base + tabs[k].off_bytes, (int)(k + 1), (size_t)tabs[k].bytes);
  for (size_t k = 0; k < tabs.size(); ++k) {
    CHECK(tabs[k].off_bytes >= 0 && tabs[k].off_bytes + tabs[k].bytes <= L.slab_bytes());
    CHECK(base[tabs[k].off_bytes] == (unsigned char)(k + 1) && base[tabs[k].off_bytes + tabs[k].bytes - 1] == (unsigned char)(k + 1));
  }
  for (size_t k = 0; k + 6 < tabs.size(); ++k) CHECK(tabs[k].off_bytes % 8 == 0);   // the double tables
  // ---- LDS -----------------------------------------------------------------------------------------------------------
  std::vector<double> lds((size_t)L.lds_total);
  unsigned char* lb = reinterpret_cast<unsigned char*>(lds.data());
  std::vector<Table> lt;
  lt.push_back({L.gs * 8LL, (long long)Mg * N * 8});
  lt.push_back({L.wblk * 8LL, 4LL * L.blk_one * 8});
  lt.push_back({L.wvec * 8LL, 4LL * 2 * L.mt_max * 8});
  lt.push_back({L.zb * 8LL, (long long)L.mt_max * kPolLongActive * 8});
  for (int o : {L.zv, L.sisq, L.di}) lt.push_back({o * 8LL, (long long)L.max_sess * 8});
  lt.push_back({L.red * 8LL, 16 * 8});
  const long long nint = 2LL * (Tm + 1) + 4LL * L.max_sess + 4LL * N + 2LL * kPolLongActive + 8;
  lt.push_back({L.ints * 8LL, nint * 4});
  if (L.cap_in_lds) lt.push_back({L.lcap * 8LL, capd * 8});
  for (size_t k = 0; k < lt.size(); ++k) std::memset(lb + lt[k].off_bytes, (int)(k + 1), (size_t)lt[k].bytes);
  for (size_t k = 0; k < lt.size(); ++k) {
    CHECK(lt[k].off_bytes + lt[k].bytes <= L.lds_bytes());
    CHECK(lb[lt[k].off_bytes] == (unsigned char)(k + 1) && lb[lt[k].off_bytes + lt[k].bytes - 1] == (unsigned char)(k + 1));
  }
  CHECK(polish_long_slab_doubles(N, Tm, K, Mg, nrow) == L.slab_total);
}

}  // namespace

int main() {
  using namespace acnqp;
  int shapes = 0;
  for (int N : {1, 3, 8, 52, 54, 63, 64})
    for (int Tm : {33, 48, 49, 64, 65, 139, 144, 256, 257, 287, 288})
      for (int K : {1, 2, 4})
        for (int Mg : {1, 8, 14, 16, 17, 20, 33, 48}) {
          const int nrow_soc = (Mg + 1) / 2, nrow_lin = Mg;   // discs (+ a peak row when Mg is odd); box rows
          one_shape(N, Tm, K, Mg, nrow_soc);
          one_shape(N, Tm, K, Mg, nrow_lin);
          shapes += 2;
        }
  CHECK(!polish_long_holds(65, 144, 1, 16, 8) && !polish_long_holds(54, 32, 1, 16, 8) && !polish_long_holds(54, 289, 1, 16, 8));
  CHECK(!polish_long_holds(64, 144, 5, 16, 8) && !polish_long_holds(54, 144, 1, 16, 0));
  // the codes: one order for (kind, p0, p1), round trip, positive
  int prev = -1;
  for (int kind = 0; kind < 4; ++kind)
    for (int p0 = 0; p0 < 64; ++p0)
      for (int p1 = 0; p1 < kPolLongMaxT; ++p1) {
        const int c = pol_code_long(kind, p0, p1);
        CHECK(c > prev || (kind == 0 && p0 == 0 && p1 == 0));
        CHECK(pol_code_long_kind(c) == kind && pol_code_long_p0(c) == p0 && pol_code_long_p1(c) == p1);
        prev = c;
      }
  const PolishLongLayout a(54, 144, 1, 16, 8), b(64, 288, 4, 32, 16);
  std::printf("{\"failures\": %d, \"shapes\": %d, \"slab_bytes_54x144\": %lld, \"lds_bytes_54x144\": %d, \"slab_bytes_64x288xK4\": %lld, "
              "\"lds_bytes_64x288xK4\": %d, \"cap_in_lds\": [%d, %d]}\n",
              failures, shapes, a.slab_bytes(), a.lds_bytes(), b.slab_bytes(), b.lds_bytes(), (int)a.cap_in_lds, (int)b.cap_in_lds);
  return failures ? 1 : 0;
}
