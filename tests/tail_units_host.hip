// Stand-alone host program over csrc/dpi_tail_units.h (tests/test_tail_split_host.py); no GPU.
//   tail_units_host sweep                              -> the properties below over the sweep; "ok <cases>"
//   tail_units_host dump nbase nblk tail order nb ng   -> the map and the rows of one launch, as text
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../deeppicarditeration_amd/csrc/dpi_tail_units.h"

using namespace dpi;

static const long long PARK_ROWS = 2048;  // DPI_PARK_MAX_BLOCKS
static long long g_cases = 0;

#define CHECK(c, ...)                         \
  do {                                        \
    if (!(c)) {                               \
      std::printf("FAIL %s: ", #c);           \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
      std::exit(1);                           \
    }                                         \
  } while (0)

// the extra rows' layout: regions in order, inside the rows, the join word 8-byte aligned
static void check_layout(int nb, int ng) {
  const int xr = tail_xrows(nb, ng);
  CHECK(nb * 256 <= tail_off_gst(nb), "nb %d", nb);
  CHECK(tail_off_gst(nb) + ng * 256 <= tail_off_bsh(nb, ng), "nb %d ng %d", nb, ng);
  CHECK(tail_off_bsh(nb, ng) + 64 <= tail_off_join(nb, ng), "nb %d ng %d", nb, ng);
  CHECK(tail_off_join(nb, ng) % 2 == 0 && tail_off_join(nb, ng) + 2 <= tail_xfloats(nb, ng), "nb %d ng %d", nb, ng);
  CHECK(xr >= 1 && tail_xfloats(nb, ng) <= xr * TAIL_PARK_ROW && tail_xfloats(nb, ng) > (xr - 1) * TAIL_PARK_ROW,
        "nb %d ng %d xr %d", nb, ng, xr);
}

static void check_cap(int nblk, long long park_rows, int nb, int ng) {
  const int cap = tail_cap(nblk, park_rows, nb, ng), xr = tail_xrows(nb, ng);
  CHECK(cap >= 0 && cap <= nblk, "nblk %d cap %d", nblk, cap);
  CHECK((long long)nblk + (long long)cap * xr <= park_rows || cap == 0, "nblk %d cap %d", nblk, cap);
  if (park_rows - nblk < xr) CHECK(cap == 0, "no free row: nblk %d cap %d", nblk, cap);
  if (cap < nblk && nblk < park_rows) CHECK((long long)nblk + (long long)(cap + 1) * xr > park_rows, "nblk %d cap %d not the most", nblk, cap);
}

static void check_launch(int nbase, int nblk, int tail, int order, int nb, int ng) {
  ++g_cases;
  const unsigned grid = tail_grid(nbase, nblk, tail);
  CHECK(grid == (unsigned)(nbase + nblk + tail), "grid");
  // bijection: every base point, whole block, I-unit and T-unit exactly once
  std::vector<unsigned char> seen(4 * (size_t)(nblk > nbase ? nblk : nbase) + 4, 0);
  std::vector<unsigned> gi(nblk, 0), gt(nblk, 0);
  const size_t stride = seen.size() / 4;
  for (unsigned g = 0; g < grid; ++g) {
    const TailUnit u = tail_unit(g, nbase, nblk, tail, order);
    CHECK(u.role >= TAIL_BASE && u.role <= TAIL_T, "g %u role %d", g, u.role);
    if (u.role == TAIL_BASE) CHECK(u.bid >= 0 && u.bid < nbase && g == (unsigned)u.bid, "g %u base %d", g, u.bid);
    if (u.role == TAIL_WHOLE) CHECK(u.bid >= 0 && u.bid < nblk - tail && g == (unsigned)(nbase + u.bid), "g %u whole %d", g, u.bid);
    if (u.role == TAIL_I || u.role == TAIL_T) {
      CHECK(u.bid >= nblk - tail && u.bid < nblk, "g %u unit of block %d", g, u.bid);
      (u.role == TAIL_I ? gi : gt)[u.bid] = g;
    }
    unsigned char& s = seen[(size_t)u.role * stride + u.bid];
    CHECK(!s, "g %u: (%d, %d) twice", g, u.role, u.bid);
    s = 1;
  }
  size_t count = 0;
  for (unsigned char s : seen) count += s;
  CHECK(count == grid, "units %zu grid %u", count, grid);
  for (int b = nblk - tail; b < nblk; ++b) {
    CHECK(seen[(size_t)TAIL_I * stride + b] && seen[(size_t)TAIL_T * stride + b], "block %d lacks a unit", b);
    // the unit order of the split part, and the same XCD (mod 8) for both where tail is a multiple of 8
    CHECK(order ? gt[b] < gi[b] : gi[b] < gt[b], "block %d order %d", b, order);
    if (tail % 8 == 0) CHECK(gi[b] % 8 == gt[b] % 8, "block %d: units %u %u", b, gi[b], gt[b]);
  }
  if (tail) {
    const TailUnit f0 = tail_unit(tail_first(nbase, nblk, tail, 0), nbase, nblk, tail, order);
    const TailUnit f1 = tail_unit(tail_first(nbase, nblk, tail, 1), nbase, nblk, tail, order);
    CHECK(f0.bid == nblk - tail && f1.bid == nblk - tail && f0.role == (order ? TAIL_T : TAIL_I) &&
              f1.role == (order ? TAIL_I : TAIL_T),
          "first units");
    CHECK(tail_first(nbase, nblk, tail, 1) + (unsigned)tail == grid, "the second units end the grid");
  }
  // rows: inside the park, beyond every block's ST row, pairwise disjoint
  const int xr = tail_xrows(nb, ng);
  long long prev_end = nblk;
  for (int b = nblk - tail; b < nblk; ++b) {
    const long long r = tail_xrow(nblk, tail, b, nb, ng);
    CHECK(r >= prev_end && r + xr <= PARK_ROWS, "block %d rows [%lld, %lld)", b, r, r + xr);
    prev_end = r + xr;
  }
}

static int sweep() {
  const int shapes[][2] = {{25, 1}, {25, 5}, {2, 1}, {1, 1}, {32, 1}, {32, 8}, {23, 8}, {24, 8}};
  for (auto& s : shapes) check_layout(s[0], s[1]);
  for (int nb = 1; nb <= 32; ++nb)
    for (int ng = 1; ng <= 8; ++ng) check_layout(nb, ng);
  for (auto& s : shapes) {
    const int nb = s[0], ng = s[1];
    for (int nblk = 1; nblk <= 2048 + 64; ++nblk) {
      check_cap(nblk, PARK_ROWS, nb, ng);
      check_cap(nblk, 0, nb, ng);
      const int cap = tail_cap(nblk, PARK_ROWS, nb, ng);
      if (nblk >= PARK_ROWS) CHECK(cap == 0, "nblk %d", nblk);
      // The flagship's row layout and the two nx = 128 layouts (two extra rows per split block, so another
      // cap and row stride): every block count, with every split count up to 320 blocks and, above, the
      // edges of the range and the multiples of 8 around them.  The other layouts (which move the rows
      // and the cap, not the grid map): the block counts up to 70 and around every multiple of 64.
      const bool first = &s == &shapes[0] || nb == 32;
      if (!first && nblk > 70 && (nblk + 1) % 64 > 2) continue;
      std::vector<int> tails;
      if (nblk <= 320 && first)
        for (int t = 0; t <= cap; ++t) tails.push_back(t);
      else
        for (int t : {0, 1, 2, 7, 8, 9, 16, cap / 2, (cap / 2) & ~7, cap & ~7, cap - 1, cap})
          if (t >= 0 && t <= cap) tails.push_back(t);
      const int nbases[] = {0, 3, nblk <= 320 ? nblk : 64};
      for (int t : tails)
        for (int order = 0; order < 2; ++order)
          for (int nbase : nbases) check_launch(nbase, nblk, t, order, nb, ng);
    }
  }
  std::printf("ok %lld\n", g_cases);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "sweep")) return sweep();
  if (argc == 8 && !std::strcmp(argv[1], "dump")) {
    const int nbase = std::atoi(argv[2]), nblk = std::atoi(argv[3]), want = std::atoi(argv[4]), order = std::atoi(argv[5]),
              nb = std::atoi(argv[6]), ng = std::atoi(argv[7]);
    const int cap = tail_cap(nblk, PARK_ROWS, nb, ng), tail = want < cap ? want : cap;
    std::printf("cap %d tail %d grid %u xrows %d gst %d bsh %d join %d\n", cap, tail, tail_grid(nbase, nblk, tail),
                tail_xrows(nb, ng), tail_off_gst(nb), tail_off_bsh(nb, ng), tail_off_join(nb, ng));
    for (unsigned g = 0; g < tail_grid(nbase, nblk, tail); ++g) {
      const TailUnit u = tail_unit(g, nbase, nblk, tail, order);
      const long long row = u.role >= TAIL_I ? tail_xrow(nblk, tail, u.bid, nb, ng) : -1;
      std::printf("%u %d %d %lld\n", g, u.role, u.bid, row);
    }
    return 0;
  }
  std::fprintf(stderr, "usage: tail_units_host sweep | dump nbase nblk tail order nb ng\n");
  return 2;
}
