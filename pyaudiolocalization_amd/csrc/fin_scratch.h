// Layout of the per-stream scratch block of the finishing column pass (pfa_cols_fin.h, pfa_fin_lean.h) and the rule that
// decides when the block must be zeroed.  Host code only, no HIP headers: tests/host/test_fin_scratch.cpp compiles it alone.
//
// The block is [done words | emax | parts | edge], each region 128-byte aligned:
//   done   Gmax x nblk x 6 unsigned   one launch number per block (per wavefront with FinArgs.pw = 4)
//   emax   2 Gmax x nblk x 12 double  a wavefront's (maximum, epoch x 2^32 + 1 + index)
//   parts  2 Gmax x nblk x 6 entries  FinPartial (104 bytes)
//   edge   2 Gmax x 4 x grid_rows double
// An entry is valid for a launch only if it carries that launch's number (`epoch`).  That holds while every word of the block
// was either zeroed or written by an earlier launch of the SAME layout: a `done` word then holds an older epoch, never the
// current one.  A launch with another layout puts its `done` words on bytes where the old layout kept maxima or partials, whose
// 32-bit words can equal any epoch; so a layout change zeroes the whole block and restarts the count, and so does the wrap.
#pragma once

#include <cstddef>

namespace pal {

constexpr size_t kFinPartialBytes = 104;        // sizeof(FinPartial), checked where the kernels define it
constexpr unsigned kFinEpochWrap = 1u << 20;    // epochs stay far below 2^21: epoch x 2^32 + index is an exact double

struct FinLayout {
  size_t off_emax, off_parts, off_edge, total;
};

inline size_t fin_align(size_t b) { return (b + 127) & ~size_t(127); }

inline FinLayout fin_layout(int Gmax, int nblk, int grid_rows) {
  FinLayout l;
  l.off_emax = fin_align(size_t(Gmax) * nblk * 6 * sizeof(unsigned));
  l.off_parts = fin_align(l.off_emax + size_t(2 * Gmax) * nblk * 12 * sizeof(double));
  l.off_edge = fin_align(l.off_parts + size_t(2 * Gmax) * nblk * 6 * kFinPartialBytes);
  l.total = l.off_edge + size_t(2 * Gmax) * 4 * grid_rows * sizeof(double);
  return l;
}

// What the layout of a launch depends on, and the block it lives in (`block`: its size; a block that grew is a new, zeroed one).
// FinArgs.pw is not part of it: it re-indexes entries inside the same regions, and the `done` region still holds only epochs.
struct FinKey {
  int gmax = 0, nblk = 0, grid_rows = 0;
  size_t block = 0;
};

inline bool operator==(const FinKey& a, const FinKey& b) {
  return a.gmax == b.gmax && a.nblk == b.nblk && a.grid_rows == b.grid_rows && a.block == b.block;
}

// true: zero the whole block and restart the epoch before this launch (`epoch`: the slot's latest launch number, 0 after a reset)
inline bool fin_must_zero(const FinKey& prev, const FinKey& now, unsigned epoch, unsigned wrap) {
  return !(prev == now) || epoch >= wrap;
}

}  // namespace pal
