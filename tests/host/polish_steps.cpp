// Stand-alone host check of what adacharge_amd/csrc/acn_qp_polish_steps.hpp states for both polish kernels and compiles on the
// host: the inverse of the packed-triangle index, for every entry of the largest capacitance matrix of the short kernel
// (128 columns) and of the long kernel (256), and the two blocking-constraint codes -- round trip of (kind, p0, p1) and
// integer order equal to the order of (kind, p0, p1) -- at the edges of what each kernel packs.  Built with
// -fsanitize=address,undefined by tests/test_polish_steps_host.py.  No GPU, no Python inside.  Prints one JSON line.
#include <cstdio>
#include <tuple>
#include <vector>

#include "acn_qp_polish_steps.hpp"

namespace {

int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; std::fprintf(stderr, "FAILED %s (line %d)\n", #c, __LINE__); } } while (0)

// every p of a packed lower triangle of n rows, against the (row, column) that was packed there
long long triangle(int n) {
  long long p = 0;
  for (int r = 0; r < n; ++r)
    for (int c = 0; c <= r; ++c, ++p) {
      const int rr = acnqp::pol_tri_row((int)p);
      if (rr != r || (int)p - rr * (rr + 1) / 2 != c) {
        ++failures;
        std::fprintf(stderr, "FAILED triangle of %d rows: p %lld is (%d, %d), got row %d\n", n, p, r, c, rr);
        return p;
      }
    }
  CHECK(p == (long long)n * (n + 1) / 2);
  return p;
}

template <class Code>
int codes(const std::vector<int>& periods) {
  using namespace acnqp;
  typedef std::tuple<int, int, int> Key;
  std::vector<Key> keys;
  for (int p0 : {0, 63})
    for (int t : periods) { keys.push_back(Key(kPolLb, p0, t)); keys.push_back(Key(kPolUb, p0, t)); }   // (EVSE, period)
  for (int p0 : {0, 63})
    for (int ks : {0, 3}) keys.push_back(Key(kPolSess, p0, ks));                                           // (EVSE, session slot)
  for (int r : {0, 31})
    for (int t : periods) keys.push_back(Key(kPolRow, r, t));                                              // (site row, period)
  for (const Key& k : keys) {
    const int c = Code::make(std::get<0>(k), std::get<1>(k), std::get<2>(k));
    CHECK(c >= 0);   // (a negative code means "no candidate" to the block-wide argmin)
    CHECK(Code::kind(c) == std::get<0>(k) && Code::p0(c) == std::get<1>(k) && Code::p1(c) == std::get<2>(k));
  }
  for (const Key& a : keys)
    for (const Key& b : keys) {
      const int ca = Code::make(std::get<0>(a), std::get<1>(a), std::get<2>(a)), cb = Code::make(std::get<0>(b), std::get<1>(b), std::get<2>(b));
      CHECK((ca < cb) == (a < b) && (ca == cb) == (a == b));
    }
  return (int)keys.size();
}

}  // namespace

int main() {
  using namespace acnqp;
  static_assert(kPolMaxSess == 128 && kPolLongMaxSess == 256, "the largest capacitance matrices this check covers");
  const long long short_entries = triangle(kPolMaxSess), long_entries = triangle(kPolLongMaxSess);
  CHECK(short_entries == 128 * 129 / 2 && long_entries == 256 * 257 / 2);
  const int short_codes = codes<PolCode8>({0, 31});
  const int long_codes = codes<PolCode12>({0, 31, 255, 256, 287});
  // the long code is the one tests/host/polish_long_slab.cpp sweeps
  CHECK(PolCode12::make(kPolRow, 31, 287) == pol_code_long(kPolRow, 31, 287));
  std::printf("{\"failures\": %d, \"triangle_entries\": [%lld, %lld], \"codes\": [%d, %d]}\n", failures, short_entries, long_entries, short_codes,
              long_codes);
  return failures ? 1 : 0;
}
