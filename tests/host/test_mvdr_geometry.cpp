// csrc/mvdr_geometry.h on the CPU: the packed triangle, the owners of k_mvdr_cov's tiles, the slices of a group and the refusal bound.
//   test_mvdr_geometry
// Built with the address and undefined-behaviour sanitizers.  Prints "ALL OK" and returns 0, or says what failed.
#include <cstdio>
#include <vector>

#include "mvdr_geometry.h"

static int failures = 0;
#define EXPECT(cond, ...)                 \
  do {                                    \
    if (!(cond)) {                        \
      std::printf("FAILED %s: ", #cond);  \
      std::printf(__VA_ARGS__);           \
      std::printf("\n");                  \
      ++failures;                         \
    }                                     \
  } while (0)

int main() {
  using namespace pal;
  // the triangle: row by row, dense, the diagonal included
  int next = 0;
  for (int i = 0; i < kMvdrMaxMics; ++i)
    for (int j = 0; j <= i; ++j) EXPECT(mvdr_tri(i, j) == next++, "tri(%d, %d)", i, j);
  EXPECT(mvdr_tri_count(kMvdrMaxMics) == next, "count %d", next);
  EXPECT(mvdr_weights_lds(kMvdrMaxMics) == 33280 && mvdr_weights_lds(kMvdrMaxMics) <= 65536, "LDS of one bin");
  // every pair j <= i < M has exactly one owner among the tiles, for every M and both tile shapes
  for (int code : {0, 44, 84}) {
    int ti = 0, tj = 0;
    mvdr_tile_shape(code, &ti, &tj);
    EXPECT(code == 44 ? (ti == 4 && tj == 4) : (ti == kMvdrTI && tj == kMvdrTJ), "tile shape %d -> %d x %d", code, ti, tj);
    for (int m = 1; m <= kMvdrMaxMics; ++m) {
      std::vector<int> owners(size_t(mvdr_tri_count(m)), 0);
      const int tiles = mvdr_tile_count(m, ti, tj);
      int last_bi = 0, last_bj = -1;
      for (int t = 0; t < tiles; ++t) {
        int bi = -1, bj = -1;
        mvdr_tile_of(t, m, ti, tj, &bi, &bj);
        EXPECT(bi >= 0 && bi < mvdr_tile_rows(m, ti) && bj >= 0 && bj < mvdr_tiles_in_row(bi, m, ti, tj), "M=%d tile %d -> (%d, %d)", m, t, bi, bj);
        EXPECT((bi == last_bi && bj == last_bj + 1) || (bi == last_bi + 1 && bj == 0), "M=%d tile %d out of order", m, t);
        last_bi = bi;
        last_bj = bj;
        int held = 0;
        for (int a = 0; a < ti; ++a)
          for (int c = 0; c < tj; ++c) {
            const int i = bi * ti + a, j = bj * tj + c;
            if (!mvdr_owned(i, j, m)) continue;
            EXPECT(j < m, "M=%d pair (%d, %d)", m, i, j);
            ++owners[size_t(mvdr_tri(i, j))];                 // (the sanitizer sees an index past the triangle)
            ++held;
          }
        EXPECT(held > 0, "M=%d tile %d (%d, %d) owns nothing", m, t, bi, bj);
      }
      for (int p = 0; p < mvdr_tri_count(m); ++p) EXPECT(owners[size_t(p)] == 1, "M=%d pair %d has %d owners", m, p, owners[size_t(p)]);
    }
  }
  EXPECT(mvdr_tile_count(64, 8, 4) == 72 && mvdr_tile_count(64, 4, 4) == 136, "tile counts at M = 64");
  EXPECT(mvdr_tile_count(1, 8, 4) == 1 && mvdr_tile_count(9, 8, 4) == 5, "tile counts at M = 1, 9");
  // slices: whole frames of one group, ascending, all of them, none beyond the group
  const int shapes[][3] = {{1, 1, 0}, {3, 1, 0}, {3, 2, 0}, {3, 3, 0}, {3, 5, 0}, {70, 0, 0}, {128, 87, 0}, {128, 0, 0}, {7, 2, 0}};
  for (const auto& sh : shapes) {
    const int q = sh[0], forced = sh[1];
    const int f0 = mvdr_slice_frames(64, 12001, forced, q);
    EXPECT(f0 >= 1 && f0 <= q, "Q=%d forced %d: %d frames per slice", q, forced, f0);
    if (forced > 0) EXPECT(f0 == (forced < q ? forced : q), "Q=%d forced %d: %d", q, forced, f0);
    for (int g = 0; g < 3; ++g) {
      int expect = g * q;
      for (int sl = 0; sl < mvdr_slice_count(q, f0); ++sl) {
        int first = -1, count = -1;
        mvdr_slice_of(g, sl, q, f0, &first, &count);
        EXPECT(first == expect && count >= 1 && count <= f0, "Q=%d f0=%d group %d slice %d: [%d, +%d)", q, f0, g, sl, first, count);
        expect = first + count;
      }
      EXPECT(expect == (g + 1) * q, "Q=%d f0=%d group %d ends at %d", q, f0, g, expect);
    }
  }
  EXPECT(mvdr_slice_frames(64, 12001, 0, 128) == 87, "the 1 GiB slice of 64 x 12 000");
  EXPECT(mvdr_slice_frames(64, size_t(1) << 21, 0, 5) == 1, "a slice holds at least one frame");
  EXPECT(mvdr_slice_frames(1, 101, 0, 100000) == kMvdrSliceMax, "a slice holds at most 32768 frames");
  // the bound: 64 microphones at 96 000 samples pass, M = 65 and a triangle above 4 GiB do not
  EXPECT(!mvdr_unsupported(64, 96001), "64 x 96 000: %llu bytes", (unsigned long long)mvdr_triangle_bytes(64, 96001));
  EXPECT(mvdr_unsupported(65, 101), "M = 65");
  EXPECT(mvdr_unsupported(64, (size_t(1) << 19) + 1), "64 x 2^19: %llu bytes", (unsigned long long)mvdr_triangle_bytes(64, (size_t(1) << 19) + 1));
  EXPECT(!mvdr_unsupported(22, (size_t(1) << 19) + 1) , "22 x 2^19");
  EXPECT(mvdr_triangle_bytes(64, 12001) == 2080ull * 12001ull * 16ull, "triangle bytes");
  if (failures) return 1;
  std::printf("ALL OK\n");
  return 0;
}
