// mvdr_geometry.h - what the MVDR beamformer (mvdr_kernels.h, Engine::mvdr_dev in beamform.hip) decides without a GPU: the index of
// the packed covariance triangle, which workgroup of k_mvdr_cov owns which tile of microphone pairs, the slices of a group's frames,
// the scratch sizes and the refusal bound.  No HIP runtime calls; tests/host/test_mvdr_geometry.cpp runs it on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define PAL_MVDR_HD __host__ __device__ inline
#else
#define PAL_MVDR_HD inline
#endif

namespace pal {

constexpr int kMvdrMaxMics = 64;          // one wavefront factors a bin, lane i owns row i
constexpr int kMvdrTI = 8, kMvdrTJ = 4;   // k_mvdr_cov: microphone pairs (i, j) per workgroup, rows x columns (the default of mvdr_tile_shape)
constexpr int kMvdrBins = 256;            // bins per workgroup of k_mvdr_cov and k_mvdr_apply: one per lane
constexpr uint64_t kMvdrTriangleBound = uint64_t(4) << 30;   // bytes of one group's covariance triangle (64 microphones at 96 000 samples)
constexpr size_t kMvdrSliceBytes = size_t(1) << 30;          // spectra of one slice of frames (Engine::beams_dev's bound)
constexpr int kMvdrSliceMax = 32768;                         // frames per slice at most

// the lower triangle with its diagonal, row by row: (0,0) (1,0) (1,1) (2,0) ...; j <= i
PAL_MVDR_HD constexpr int mvdr_tri(int i, int j) { return i * (i + 1) / 2 + j; }
PAL_MVDR_HD constexpr int mvdr_tri_count(int m) { return m * (m + 1) / 2; }

// k_mvdr_cov's tiles of ti x tj microphone pairs: block row bi holds the microphones bi ti .. bi ti + ti - 1 (below M), block column
// bj the microphones bj tj .. bj tj + tj - 1; a tile exists where it holds a pair with j <= i.  Tiles are numbered row by row.
PAL_MVDR_HD constexpr int mvdr_tile_rows(int m, int ti) { return (m + ti - 1) / ti; }
PAL_MVDR_HD constexpr int mvdr_tiles_in_row(int bi, int m, int ti, int tj) {
  return ((bi * ti + ti < m ? bi * ti + ti : m) - 1) / tj + 1;   // columns up to the row's last microphone
}
PAL_MVDR_HD constexpr int mvdr_tile_count(int m, int ti, int tj) {
  int n = 0;
  for (int bi = 0; bi < mvdr_tile_rows(m, ti); ++bi) n += mvdr_tiles_in_row(bi, m, ti, tj);
  return n;
}
PAL_MVDR_HD void mvdr_tile_of(int t, int m, int ti, int tj, int* bi, int* bj) {
  int r = 0;
  while (t >= mvdr_tiles_in_row(r, m, ti, tj)) t -= mvdr_tiles_in_row(r++, m, ti, tj);
  *bi = r;
  *bj = t;
}
// the pair (i0 + a, j0 + c) of a tile is the tile's to accumulate and store
PAL_MVDR_HD constexpr bool mvdr_owned(int i, int j, int m) { return i < m && j <= i; }
// PAL_MVDR_TILE: 44 (anything else: the default, 8 x 4) -> ti, tj.  (8 x 8 was compiled and left out: 256 registers and 32 spilled.)
inline void mvdr_tile_shape(int code, int* ti, int* tj) {
  *ti = code == 44 ? 4 : kMvdrTI;
  *tj = kMvdrTJ;
}

// slices of whole frames that never straddle a group: F0 frames per slice (the last slice of a group holds the rest)
inline int mvdr_slice_frames(int m, size_t h, int forced, int q) {
  size_t per = kMvdrSliceBytes / (size_t(m) * h * 16);
  if (forced > 0) per = size_t(forced);
  per = per < 1 ? 1 : (per > size_t(kMvdrSliceMax) ? size_t(kMvdrSliceMax) : per);
  return int(per > size_t(q) ? size_t(q) : per);
}
inline int mvdr_slice_count(int q, int f0) { return (q + f0 - 1) / f0; }
// frames [first, first + count) of the call that slice `sl` of group `g` holds
inline void mvdr_slice_of(int g, int sl, int q, int f0, int* first, int* count) {
  *first = g * q + sl * f0;
  *count = q - sl * f0 < f0 ? q - sl * f0 : f0;
}

inline uint64_t mvdr_triangle_bytes(int m, size_t h) { return uint64_t(mvdr_tri_count(m)) * uint64_t(h) * 16; }
inline bool mvdr_unsupported(int m, size_t h) { return m > kMvdrMaxMics || mvdr_triangle_bytes(m, h) > kMvdrTriangleBound; }
inline size_t mvdr_weights_lds(int m) { return size_t(mvdr_tri_count(m)) * 16; }   // k_mvdr_weights: the triangle of one bin

}  // namespace pal
