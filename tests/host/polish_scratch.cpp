// Stand-alone host check of the scratch buffer of a polished launch (adacharge_amd/csrc/acn_qp_polplan.hpp: PolishScratch):
// for every (kind, shape, batch, caller_has_y) of a grid the buffer is malloc'ed at exactly the `total` the plan states,
// carved up as acn_qp_api.hip carves it, every region written from its first to its last element with its own element type
// (int32_t counters, list and saved status; double multipliers and slabs) and a pattern of its own, and all of them read
// back afterwards.  Built with -fsanitize=address,undefined by tests/test_polish_plan.py: a region that overruns the
// buffer, or two that overlap, fail the run.  No GPU, no Python inside.  Prints one JSON line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "acn_qp_polplan.hpp"

namespace {

int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; std::fprintf(stderr, "FAILED %s (line %d)\n", #c, __LINE__); } } while (0)

template <typename T>
struct Region { T* p; size_t n; T first; };

template <typename T>
void fill(const Region<T>& r) { for (size_t k = 0; k < r.n; ++k) r.p[k] = (T)(r.first + (T)k); }
template <typename T>
size_t wrong(const Region<T>& r) {
  size_t bad = 0;
  for (size_t k = 0; k < r.n; ++k) bad += r.p[k] != (T)(r.first + (T)k);
  return bad;
}

size_t largest = 0;

void one(acnqp::PolishKind kind, const acnqp::SiteShape& s, int Tm, int K, int batch, bool has_y, bool own_stream) {
  using namespace acnqp;
  const int grid = polish_grid(kind, batch, own_stream, 256);
  const size_t sbytes = polish_slab_bytes(kind, s, Tm, K, grid);
  const PolishScratch sc(kind, batch, s.Mg, Tm, has_y, sbytes);
  CHECK((kind == PolishKind::on_chip) == (sbytes == 0) && sbytes % 8 == 0);
  CHECK(sc.ctr == 0 && sc.list == PolishScratch::kCtrBytes && sc.list <= sc.saved && sc.saved <= sc.y && sc.y <= sc.slab && sc.slab <= sc.total);
  for (size_t o : {sc.ctr, sc.list, sc.saved, sc.y, sc.slab}) CHECK(o % 256 == 0);
  largest = sc.total > largest ? sc.total : largest;
  char* base = static_cast<char*>(std::malloc(sc.total));
  CHECK(base != nullptr);
  if (!base) return;
  // as reserve_polish (acn_qp_api.hip) hands the regions out; the list's region whole, as the launch alongside clears it
  const Region<int32_t> ctr{reinterpret_cast<int32_t*>(base + sc.ctr), PolishScratch::kCtrBytes / sizeof(int32_t), 0x11000000};
  const Region<int32_t> list{reinterpret_cast<int32_t*>(base + sc.list), sc.list_bytes / sizeof(int32_t), 0x22000000};
  const Region<int32_t> saved{reinterpret_cast<int32_t*>(base + sc.saved), kind == PolishKind::wide ? (size_t)batch : 0, 0x33000000};
  const Region<double> y{reinterpret_cast<double*>(base + sc.y), has_y ? 0 : (size_t)batch * s.Mg * Tm, 1.0e9};
  const Region<double> slab{reinterpret_cast<double*>(base + sc.slab), sbytes / sizeof(double), -0.5};
  CHECK(list.n >= (size_t)batch && kPolCtrPolishQueue < (int)ctr.n && kPolCtrResumeQueue < (int)ctr.n && kPolCtrListLength < (int)ctr.n && kPolCtrRetired < (int)ctr.n);
  fill(ctr); fill(list); fill(saved); fill(y); fill(slab);
  CHECK(wrong(ctr) == 0 && wrong(list) == 0 && wrong(saved) == 0 && wrong(y) == 0 && wrong(slab) == 0);
  // the last byte of the last region is the last byte of the buffer, but for the rounding of the on-chip kind's last region
  const size_t end = sbytes ? sc.slab + sbytes : (y.n ? sc.y + y.n * sizeof(double) : sc.list + sc.list_bytes);
  CHECK(end <= sc.total && sc.total - end < 256 && (sbytes == 0 || end == sc.total));
  std::free(base);
}

}  // namespace

int main() {
  using namespace acnqp;
  int combos = 0, by_kind[3] = {0, 0, 0};
  const int batches[] = {1, 2, 63, 64, 65, 2048};
  // sites (M, cone, peak): box rows, discs with a peak row
  const int sites[2][3] = {{10, ACNQP_CONE_LINEAR, 0}, {10, ACNQP_CONE_SOC, 1}};
  struct Grid { PolishKind kind; int N[4], nN, T[5], nT, K[2]; };
  const Grid grids[3] = {{PolishKind::on_chip, {1, 8, 54, 64}, 4, {1, 12, 16, 17, 32}, 5, {1, 1}},
                         {PolishKind::long_horizon, {8, 54, 64, 0}, 3, {33, 48, 49, 96, 0}, 4, {1, 4}},
                         {PolishKind::wide, {65, 80, 130, 0}, 3, {1, 12, 47, 48, 0}, 4, {1, 4}}};
  for (int g = 0; g < 3; ++g)
    for (int in = 0; in < grids[g].nN; ++in)
      for (int it = 0; it < grids[g].nT; ++it)
        for (int si = 0; si < 2; ++si) {
          const int K = grids[g].K[si];   // (one session slot with the box rows, the kind's most with the discs)
          const SiteShape s = site_shape(grids[g].N[in], sites[si][0], sites[si][1], sites[si][2], 0, 0);
          for (int batch : batches)
            for (int has_y = 0; has_y < 2; ++has_y) {
              one(grids[g].kind, s, grids[g].T[it], K, batch, has_y != 0, (combos & 1) != 0);
              ++combos;
              ++by_kind[g];
            }
        }
  std::printf("{\"failures\": %d, \"combinations\": %d, \"by_kind\": [%d, %d, %d], \"largest_total\": %zu}\n", failures, combos, by_kind[0],
              by_kind[1], by_kind[2], largest);
  return failures ? 1 : 0;
}
