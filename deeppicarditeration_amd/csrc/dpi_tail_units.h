// The unit map of a parking path launch whose last path blocks run as two workgroups each
// (dpi_device.h paths_body, "tail units"): grid index -> (role, block id), the park rows of a split
// block, the cap on the split count and the layout of a split block's extra rows.  Plain integer
// functions, no HIP call: the host (label_args, the launches) and the kernel read the same map, and
// tests/tail_units_host.hip sweeps it without a device.
//
// Grid order of a launch over nblk = n nbp path blocks, the last `tail` of them split:
//   [nbase base blocks][nblk - tail whole blocks][tail first units][tail second units]
// order 0: the first units are the I-units (integral rollout + MLP), the second the T-units (terminal
// rollout); order 1: T-units first.  Unit k of either kind belongs to block nblk - tail + k, so the two
// units of a block sit `tail` grid indices apart: congruent mod 8 — dealt to the same XCD — whenever
// tail is a multiple of 8.
//
// Park rows (PARK_ROW floats each, park_rows of them): row b < nblk holds block b's terminal sums as
// before; split block k owns the tail_xrows() rows from nblk + k tail_xrows() on, laid out (in floats)
//   [S: dim-block j < nb][lane 64][4] | [gst: statistic c < ng][wave 4][lane 64] | [bsh: lane 64] | join word (64 bit)
// so a call splits at most tail_cap() blocks: what the rows beside its own nblk hold.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DPI_TAIL_HD __host__ __device__
#else
#define DPI_TAIL_HD
#endif

namespace dpi {

constexpr int TAIL_PARK_ROW = 4 * 8 * 64 * 4;  // floats of a park row (dpi_device.h PARK_ROW)
enum TailRole { TAIL_BASE = 0, TAIL_WHOLE = 1, TAIL_I = 2, TAIL_T = 3 };

// offsets (floats) inside a split block's extra rows; nb: dim-blocks of 4, ng: g statistics per wave
DPI_TAIL_HD constexpr int tail_off_gst(int nb) { return nb * 256; }
DPI_TAIL_HD constexpr int tail_off_bsh(int nb, int ng) { return (nb + ng) * 256; }
DPI_TAIL_HD constexpr int tail_off_join(int nb, int ng) { return (nb + ng) * 256 + 64; }
DPI_TAIL_HD constexpr int tail_xfloats(int nb, int ng) { return tail_off_join(nb, ng) + 2; }
DPI_TAIL_HD constexpr int tail_xrows(int nb, int ng) { return (tail_xfloats(nb, ng) + TAIL_PARK_ROW - 1) / TAIL_PARK_ROW; }

// the most blocks a call of nblk path blocks may split: every split block's extra rows lie in the
// rows of the park that no block of the call uses
DPI_TAIL_HD constexpr int tail_cap(long long nblk, long long park_rows, int nb, int ng) {
  if (nblk <= 0 || nblk >= park_rows) return 0;
  const long long room = (park_rows - nblk) / tail_xrows(nb, ng);
  return (int)(room < nblk ? room : nblk);
}
// first extra row of split block bid (nblk - tail <= bid < nblk)
DPI_TAIL_HD constexpr long long tail_xrow(int nblk, int tail, int bid, int nb, int ng) {
  return (long long)nblk + (long long)(bid - (nblk - tail)) * tail_xrows(nb, ng);
}

DPI_TAIL_HD constexpr unsigned tail_grid(int nbase, int nblk, int tail) { return (unsigned)nbase + (unsigned)nblk + (unsigned)tail; }
// grid index of the first unit of the split part (the unit offset of a launch of its own)
DPI_TAIL_HD constexpr unsigned tail_first(int nbase, int nblk, int tail, int second) {
  return (unsigned)nbase + (unsigned)(nblk - tail) + (second ? (unsigned)tail : 0u);
}

struct TailUnit {
  int role;  // TailRole
  int bid;   // base blocks: the point; else the path block
};
DPI_TAIL_HD constexpr TailUnit tail_unit(unsigned g, int nbase, int nblk, int tail, int order) {
  if (g < (unsigned)nbase) return TailUnit{TAIL_BASE, (int)g};
  const int u = (int)(g - (unsigned)nbase), whole = nblk - tail;
  if (u < whole) return TailUnit{TAIL_WHOLE, u};
  const int k = u - whole, second = k >= tail;
  return TailUnit{(second != 0) == (order != 0) ? TAIL_I : TAIL_T, whole + (second ? k - tail : k)};
}

}  // namespace dpi
