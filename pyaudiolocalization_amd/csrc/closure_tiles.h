// closure_tiles.h - what the closure check (closure.hip) and the consensus (consensus.hip) share: the row-major pair index, the tiles of
// 16 x 16 pairs on and above the diagonal of a frame's microphone matrix, the fill of a tile's lag rows in LDS and the vote loop over
// third microphones.  No HIP runtime calls; everything but the LDS fill also compiles for the host, where
// tests/host/test_closure_tiles.cpp runs it against plain loops.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define PAL_CT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PAL_CT_HD inline
#endif

namespace pal {

constexpr int kPairTile = 16;                  // pairs per tile side: 256 lanes, one per pair
constexpr int kTileThreads = 256;
constexpr int kTileMaxMics = 256;
constexpr int kLagStride = kTileMaxMics + 1;   // odd: the sixteen j-rows a wavefront reads at one k sit in sixteen banks.  2 x 16 x 257 x 4 B = 32 896 B
static_assert(kTileThreads == kPairTile * kPairTile && kTileThreads >= kTileMaxMics, "one lane per pair of a tile, one per microphone");

// pair (i, j), i < j, of M microphones is row pair_row(i, M) + j of a frame's table (I = int64_t where M * M may pass int32)
template <class I>
PAL_CT_HD I pair_row(I i, I M) { return i * M - i * (i + 1) / 2 - i - 1; }

// tile t of a frame -> (ti, tj): tile row ti holds the tiles tj = ti .. tiles - 1 (uniform over a workgroup)
PAL_CT_HD void tile_of(int t, int tiles, int& ti, int& tj) {
  ti = 0;
  while (t >= tiles - ti) { t -= tiles - ti; ++ti; }
  tj = ti + t;
}

// array index k of a frame of lm1 + 1 samples -> lag; outside 0 .. 2 lm1 sets `bad` and enters as lag 0, so no sum can overflow
PAL_CT_HD int lag_of_index(int k, int lm1, bool& bad) {
  const bool ok = k >= 0 && k <= 2 * lm1;
  bad |= !ok;
  return ok ? k - lm1 : 0;
}

// v[c] = #{k not in {i, j} : |ri[k] - rj[k] - lag_c| <= tol} for lo[c] = lag_c - tol and tol2 = 2 tol: one unsigned compare per test
// (|lag| < 2^24 and tol <= 2^20 keep every difference far inside int32).  ri, rj: rows i and j of an antisymmetric lag matrix with a
// zero diagonal.  The loop counts every k; at k = i and at k = j the difference is ri[j] for every candidate, so v[c] starts two below
// zero where that one passes the test (a `k != i && k != j` in the loop costs a third more instructions per k).
template <int KT>
PAL_CT_HD void tile_votes(const int32_t* ri, const int32_t* rj, int M, int j, const int (&lo)[KT], unsigned tol2, int (&v)[KT]) {
  constexpr int kUnroll = KT >= 8 ? 2 : 4;
#pragma unroll
  for (int c = 0; c < KT; ++c) v[c] = unsigned(ri[j] - lo[c]) <= tol2 ? -2 : 0;
#pragma unroll kUnroll
  for (int k = 0; k < M; ++k) {
    const int d = ri[k] - rj[k];
#pragma unroll
    for (int c = 0; c < KT; ++c) v[c] += unsigned(d - lo[c]) <= tol2;
  }
}

#if defined(__HIPCC__) || defined(__CUDACC__)
// rows ti * 16 .. + 15 and tj * 16 .. + 15 of the M x M lag matrix A into LDS (zeros past row M - 1); the caller's barrier follows
__device__ inline void load_lag_tile(const int32_t* A, int M, int ti, int tj, int32_t* rows_i, int32_t* rows_j) {
  for (int r = 0; r < kPairTile; ++r) {
    const int gi = ti * kPairTile + r, gj = tj * kPairTile + r;
    for (int k = threadIdx.x; k < M; k += kTileThreads) {
      rows_i[r * kLagStride + k] = gi < M ? A[size_t(gi) * M + k] : 0;
      rows_j[r * kLagStride + k] = gj < M ? A[size_t(gj) * M + k] : 0;
    }
  }
}
#endif

}  // namespace pal
