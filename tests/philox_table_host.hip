// Host program of tests/test_philox_table_host.py: the table form of Philox4x32-10 (dpi_rng.h: table
// entry + lane invariant + per-call tail) on counters read from stdin.
// in:  one counter per line, "c0 m i c3 k0 k1" (decimal uint32)
// out: its four output words, "w0 w1 w2 w3"
#include <cstdio>

#include "../deeppicarditeration_amd/csrc/dpi_rng.h"

int main() {
  unsigned c0, m, i, c3, k0, k1;
  while (std::scanf("%u %u %u %u %u %u", &c0, &m, &i, &c3, &k0, &k1) == 6) {
    const dpi::PhiloxLane li = dpi::philox_lane_invariant(m, i, k0);
    const dpi::u32e4 e = dpi::philox_table_entry(c0, i, c3, k0, k1);
    const dpi::u32x4 w = dpi::philox4x32_10_tail(li, e, k0, k1);
    std::printf("%u %u %u %u\n", w.x, w.y, w.z, w.w);
  }
  return 0;
}
