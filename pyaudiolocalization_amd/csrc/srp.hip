// srp.hip - steered-response power (SRP-PHAT) map from all-pairs GCC-PHAT rows (pal_gcc_phat_all_pairs_strips*, pal_srp_map*,
// pal_srp_peaks*, pal_srp_zoom*; specification: pyaudiolocalization_amd/srp.py; arithmetic: srp_math.h).  Built with -ffp-contract=off.
//
//   k_srp_strips   one lane per output sample of strips[rows][2T+1]: the 2W+1 neighbours of the row around the sample's lag, weighted
//                  by the triangle and added in the specification's order.  It runs behind a frame slice of the pair pipeline, whose
//                  rows [slice pairs][2L-1] sit in engine scratch (pal_api.hip: strips_dev; frames go through in slices whose rows stay
//                  under about 1 GiB, never less than one frame - one frame of 64 microphones and L = 44 100 alone is 1.4 GB).  A row's
//                  samples come from HBM once (the neighbours of one sample are the next lanes' samples: L1 / L2 serve them), coalesced
//                  apart from the wrap at lag 0;
//   k_srp_map      one lane per grid cell, a workgroup takes 256 consecutive linear indices of one frame: with iz fastest, neighbouring
//                  lanes' lags for one pair differ by a sample or two, so a wavefront's 64 reads of a pair touch a few cache lines of
//                  that pair's strip.  Microphones go through in tiles of 16 (closure_tiles.h: kPairTile): the 16 distances of tile ti
//                  sit in LDS as d[mic][lane] - a lane reads only what it wrote, so there is no barrier - and the 16 of tile tj >= ti in
//                  registers, with the loop over them unrolled; a distance is computed once per tile pass, not once per pair:
//                  16 (tiles + tiles (tiles + 1) / 2) square roots per cell against M (M - 1) / 2 lags.  The sum runs in the fixed order
//                  (ti, tj, i, j), one rounded product and one rounded addition per term: the same input gives the same bytes whatever B
//                  is.  Clipped terms are counted per lane, added up in LDS and leave with one 64-bit integer atomic per workgroup.  No
//                  floating-point atomics, no waits between workgroups, no scratch;
//   k_srp_peaks    one workgroup of 1024 per frame over the stored map: marks the peaks by the neighbourhood rule (one byte per cell in
//                  engine scratch), then K selection passes, each the block maximum - in the order power descending, index ascending - of
//                  the marks behind the previous pass's pick; writes peaks[B][K] and the frame's summary.  The passes are
//                  srp_select.h's, shared with the direction map's k_srp_doa_peaks (srp_doa.hip);
//   k_srp_zoom     one workgroup of 256 per (frame, seed) runs every level of the coarse-to-fine zoom (srp.zoom): a level's Z^3 cells in
//                  chunks of 256, one lane per cell, with k_srp_map's tile scheme and the strip read at the fractional lag (two samples,
//                  blended); the level's best cell by one block reduction, the next box through LDS.  The cell body is a second copy
//                  of the map's loop with another term: one body with the term as a functor cost k_srp_map two VGPRs.  No atomics on global memory, no
//                  scratch.
#include "closure_tiles.h"
#include "engine.h"
#include "srp_math.h"
#include "srp_select.h"
#include "wave_reduce.h"

namespace pal {

static_assert(kSrpMaxSmooth == PAL_SRP_MAX_SMOOTH && kSrpMaxPeaks == PAL_SRP_MAX_PEAKS && kSrpMaxRadius == PAL_SRP_MAX_RADIUS,
              "srp_math.h and pal_hip.h state the same limits");
static_assert(sizeof(pal_srp_grid) == 64 && sizeof(pal_srp_peak) == 40 && sizeof(pal_srp_frame) == 16, "record sizes of pal_hip.h");
static_assert(kSrpMaxZoomCells == PAL_SRP_MAX_ZOOM_CELLS && kSrpMaxZoomLevels == PAL_SRP_MAX_ZOOM_LEVELS, "the zoom's limits");
static_assert(sizeof(pal_srp_zoom_record) == 48, "record size of pal_hip.h");

struct SrpStripArgs {
  const double* rows;   // [nrows][n]
  double* out;          // [nrows][2T+1]
  int64_t total;        // nrows * (2T+1)
  int n, T, W;
};

__global__ __launch_bounds__(kSrpThreads) void k_srp_strips(SrpStripArgs a) {
  const int64_t at = int64_t(blockIdx.x) * kSrpThreads + threadIdx.x;
  if (at >= a.total) return;
  const int width = 2 * a.T + 1;
  const int64_t row = at / width;
  const int s = int(at - row * width) - a.T;
  a.out[at] = srp_smooth(a.rows + size_t(row) * size_t(a.n), a.n, s, a.W);   // |s| + W <= L - 1 < n (srp_strips_check)
}

struct SrpMapArgs {
  const double* strips;            // [B][P][2T+1]
  const double* weights;           // [B][P] or nullptr
  const double* mics;              // [M][3]
  double* power;                   // [B][G]
  unsigned long long* clipped;     // [B], zeroed before the launch
  double lo[3], step[3];
  double fs, c, inv_c;
  int ny, nz, G, M, P, T, tiles, blocks;   // blocks: workgroups per frame
};

__global__ __launch_bounds__(kSrpThreads) void k_srp_map(SrpMapArgs a) {
  __shared__ double d_i[kPairTile * kSrpThreads];   // d[mic of tile ti][lane]: 32 KiB
  __shared__ int clip_sum;
  const int tid = threadIdx.x, b = blockIdx.x / a.blocks, M = a.M;
  const int g0 = (blockIdx.x % a.blocks) * kSrpThreads + tid;
  const bool active = g0 < a.G;
  const int g = active ? g0 : a.G - 1;            // a lane past the grid computes the last cell and writes nothing
  if (tid == 0) clip_sum = 0;
  int ix, iy, iz;
  srp_cell(g, a.ny, a.nz, ix, iy, iz);
  const double x = srp_coord(a.lo[0], a.step[0], ix), y = srp_coord(a.lo[1], a.step[1], iy), z = srp_coord(a.lo[2], a.step[2], iz);
  const int width = 2 * a.T + 1;
  const double* st = a.strips + size_t(b) * size_t(a.P) * size_t(width) + a.T;
  const double* wt = a.weights ? a.weights + size_t(b) * size_t(a.P) : nullptr;
  double acc = 0.0;
  int clip = 0;
  for (int ti = 0; ti < a.tiles; ++ti) {
    for (int r = 0; r < kPairTile; ++r) {
      const int i = ti * kPairTile + r;
      if (i < M) d_i[r * kSrpThreads + tid] = srp_distance(x, y, z, a.mics[3 * i], a.mics[3 * i + 1], a.mics[3 * i + 2]);
    }
    for (int tj = ti; tj < a.tiles; ++tj) {
      double d_j[kPairTile];
#pragma unroll
      for (int r = 0; r < kPairTile; ++r) {
        const int j = tj * kPairTile + r;
        d_j[r] = j < M ? srp_distance(x, y, z, a.mics[3 * j], a.mics[3 * j + 1], a.mics[3 * j + 2]) : 0.0;
      }
      for (int r = 0; r < kPairTile; ++r) {
        const int i = ti * kPairTile + r;
        if (i >= M - 1) break;
        const double di = d_i[r * kSrpThreads + tid];
        const int64_t row0 = pair_row(int64_t(i), int64_t(M));
#pragma unroll
        for (int q = 0; q < kPairTile; ++q) {
          const int j = tj * kPairTile + q;
          if (j > i && j < M) {                    // uniform over the workgroup
            const double lag = srp_lag(di, d_j[q], a.fs, a.c, a.inv_c);
            if (srp_clipped(lag, a.T)) {
              ++clip;
            } else {
              double v = st[size_t(row0 + j) * size_t(width) + int(lag)];
              if (wt) v = wt[row0 + j] * v;
              acc = acc + v;
            }
          }
        }
      }
    }
  }
  __syncthreads();                                 // clip_sum is zero
  if (active) {
    a.power[size_t(b) * size_t(a.G) + g] = acc;
    if (clip) atomicAdd(&clip_sum, clip);
  }
  __syncthreads();
  if (tid == 0 && clip_sum) atomicAdd(a.clipped + b, (unsigned long long)clip_sum);
}

struct SrpPeakArgs {
  const double* power;                  // [B][G]
  unsigned char* marks;                 // [B][G] (K > 0)
  pal_srp_peak* peaks;                  // [B][K] or nullptr
  pal_srp_frame* summary;               // [B] or nullptr
  const unsigned long long* clipped;    // [B] or nullptr (then 0)
  double lo[3], step[3];
  int nx, ny, nz, G, K, R;
};

__global__ __launch_bounds__(kSrpPeakThreads) void k_srp_peaks(SrpPeakArgs a) {
  __shared__ double best_p[kSrpPeakThreads];
  __shared__ int best_g[kSrpPeakThreads];
  const int tid = threadIdx.x, b = blockIdx.x, G = a.G;
  const double* power = a.power + size_t(b) * size_t(G);
  unsigned char* marks = a.marks + size_t(b) * size_t(G);
  if (a.K > 0) {
    for (int g = tid; g < G; g += kSrpPeakThreads) {
      int ix, iy, iz;
      srp_cell(g, a.ny, a.nz, ix, iy, iz);
      marks[g] = srp_is_peak(power, a.nx, a.ny, a.nz, ix, iy, iz, a.R) ? 1 : 0;
    }
  }
  __syncthreads();
  srp_select_peaks(power, marks, G, a.K, a.peaks ? a.peaks + size_t(b) * size_t(a.K) : nullptr, a.summary ? a.summary + b : nullptr,
                   a.clipped ? a.clipped + b : nullptr, best_p, best_g, [&](int g, pal_srp_peak& rec) {
                     int ix, iy, iz;
                     srp_cell(g, a.ny, a.nz, ix, iy, iz);
                     rec.x = srp_coord(a.lo[0], a.step[0], ix);
                     rec.y = srp_coord(a.lo[1], a.step[1], iy);
                     rec.z = srp_coord(a.lo[2], a.step[2], iz);
                   });
}

struct SrpZoomArgs {
  const double* strips;            // [B][P][2T+1]
  const double* weights;           // [B][P] or nullptr
  const double* mics;              // [M][3]
  const pal_srp_peak* seeds;       // [B][K]
  pal_srp_zoom_record* out;        // [B][K]
  double half0[3];
  double fs, c;
  int M, P, T, tiles, K, Z, levels;
};

// the power of one point by the zoom's rule (srp_zoom_term), summed in the order of srp.tile_order - k_srp_map's tile scheme with
// another term: tile ti's distances in this lane's column of d_i, tile tj's in registers.  -> clipped terms of this point
__device__ __forceinline__ int zoom_cell(const SrpZoomArgs& a, const double* st, const double* wt, double* d_i, int tid, double x, double y,
                                         double z, double& power) {
  const int M = a.M, width = 2 * a.T + 1;
  double acc = 0.0;
  int clip = 0;
  for (int ti = 0; ti < a.tiles; ++ti) {
    for (int r = 0; r < kPairTile; ++r) {
      const int i = ti * kPairTile + r;
      if (i < M) d_i[r * kSrpThreads + tid] = srp_distance(x, y, z, a.mics[3 * i], a.mics[3 * i + 1], a.mics[3 * i + 2]);
    }
    for (int tj = ti; tj < a.tiles; ++tj) {
      double d_j[kPairTile];
#pragma unroll
      for (int r = 0; r < kPairTile; ++r) {
        const int j = tj * kPairTile + r;
        d_j[r] = j < M ? srp_distance(x, y, z, a.mics[3 * j], a.mics[3 * j + 1], a.mics[3 * j + 2]) : 0.0;
      }
      for (int r = 0; r < kPairTile; ++r) {
        const int i = ti * kPairTile + r;
        if (i >= M - 1) break;
        const double di = d_i[r * kSrpThreads + tid];
        const int64_t row0 = pair_row(int64_t(i), int64_t(M));
#pragma unroll
        for (int q = 0; q < kPairTile; ++q) {
          const int j = tj * kPairTile + q;
          if (j > i && j < M) {                    // uniform over the workgroup
            double v;
            if (!srp_zoom_term(st + size_t(row0 + j) * size_t(width), a.T, di, d_j[q], a.fs, a.c, &v)) {
              ++clip;
            } else {
              if (wt) v = wt[row0 + j] * v;
              acc = acc + v;
            }
          }
        }
      }
    }
  }
  power = acc;
  return clip;
}

// one workgroup per (frame, seed) runs every level: the level's centre and half-extent sit in LDS, its Z^3 cells go through in chunks
// of 256 (one lane per cell), every lane keeps its best (power, index) by srp_before with NaN never entered, one block reduction picks
// the level's best and thread 0 writes the next level's box.  `stop` is read from LDS by every lane after a barrier, so the whole
// workgroup leaves together.  The record belongs to this workgroup: no global atomics.
__global__ __launch_bounds__(kSrpThreads) void k_srp_zoom(SrpZoomArgs a) {
  __shared__ double d_i[kPairTile * kSrpThreads];   // d[mic of tile ti][lane]: 32 KiB
  __shared__ double ctr[3], half[3];
  __shared__ double wave_p[kSrpThreads / 64];
  __shared__ int wave_g[kSrpThreads / 64];
  __shared__ unsigned long long clip_sum;        // 16^3 cells x P terms a level pass int32 from M = 1025 on
  __shared__ int stop;
  const int tid = threadIdx.x, b = blockIdx.x / a.K, Z = a.Z, G = Z * Z * Z;
  pal_srp_zoom_record rec;                          // thread 0's
  rec.x = rec.y = rec.z = rec.power = 0.0;
  rec.clipped = 0;
  rec.seed = -1;
  rec.levels = 0;
  if (tid == 0) {
    const pal_srp_peak seed = a.seeds[blockIdx.x];
    clip_sum = 0;
    stop = srp_zoom_absent(seed.index) ? 1 : 0;
    if (!stop) {
      rec.x = ctr[0] = seed.x;
      rec.y = ctr[1] = seed.y;
      rec.z = ctr[2] = seed.z;
      rec.seed = seed.index;
      for (int ax = 0; ax < 3; ++ax) half[ax] = a.half0[ax];
    }
  }
  __syncthreads();
  const bool absent = stop != 0;                    // uniform
  const int width = 2 * a.T + 1;
  const double* st = a.strips + size_t(b) * size_t(a.P) * size_t(width) + a.T;
  const double* wt = a.weights ? a.weights + size_t(b) * size_t(a.P) : nullptr;
  for (int level = 0; level < a.levels && !absent; ++level) {
    double lo[3], step[3];
    for (int ax = 0; ax < 3; ++ax) {
      double hi;
      srp_zoom_box(ctr[ax], half[ax], lo[ax], hi);
      step[ax] = srp_step(lo[ax], hi, Z);
    }
    double my_p = 0.0;
    int my_g = -1, clip = 0;
    for (int g0 = tid; g0 - tid < G; g0 += kSrpThreads) {   // every lane runs every chunk
      const bool active = g0 < G;
      const int g = active ? g0 : G - 1;            // a lane past Z^3 computes the last cell and takes no part in the reduction
      int ix, iy, iz;
      srp_cell(g, Z, Z, ix, iy, iz);
      double p;
      const int c = zoom_cell(a, st, wt, d_i, tid, srp_coord(lo[0], step[0], ix), srp_coord(lo[1], step[1], iy),
                              srp_coord(lo[2], step[2], iz), p);
      if (active) {
        clip += c;
        if (p == p && (my_g < 0 || srp_before(p, g, my_p, my_g))) { my_p = p; my_g = g; }
      }
    }
    wave_arg63(my_p, my_g, [](double pa, int ga, double pb, int gb) { return srp_before(pa, ga, pb, gb); });   // lane 63 holds the wave's best
    if ((tid & 63) == 63) {
      wave_p[tid >> 6] = my_p;
      wave_g[tid >> 6] = my_g;
    }
    if (clip) atomicAdd(&clip_sum, (unsigned long long)clip);   // a lane's own count: at most 16 cells x P < 2^31
    __syncthreads();
    if (tid == 0) {
      double best_p = wave_p[0];
      int best_g = wave_g[0];
      for (int w = 1; w < kSrpThreads / 64; ++w)
        if (wave_g[w] >= 0 && (best_g < 0 || srp_before(wave_p[w], wave_g[w], best_p, best_g))) { best_p = wave_p[w]; best_g = wave_g[w]; }
      rec.clipped += int64_t(clip_sum);
      clip_sum = 0;
      if (srp_zoom_stops(best_g)) {
        stop = 1;                                   // the record keeps the centre this level started from
        rec.power = __builtin_nan("");
      } else {
        int ix, iy, iz;
        srp_cell(best_g, Z, Z, ix, iy, iz);
        const int cell[3] = {ix, iy, iz};
        double c3[3];
        for (int ax = 0; ax < 3; ++ax) {
          c3[ax] = srp_coord(lo[ax], step[ax], cell[ax]);
          ctr[ax] = c3[ax];
          half[ax] = step[ax];                      // srp_zoom_next_half(lo, hi, Z): one cell of this level
        }
        rec.x = c3[0];
        rec.y = c3[1];
        rec.z = c3[2];
        rec.power = best_p;
        rec.levels = level + 1;
      }
    }
    __syncthreads();                                // the next box, or stop, is in LDS; wave_p / wave_g are free again
    if (stop) break;                                // uniform
  }
  if (tid == 0) a.out[blockIdx.x] = rec;
}

// ---- host side ----

static bool finite3(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// the grid's own checks -> G
static int grid_check(Engine* e, const pal_srp_grid* grid, int* G) {
  if (!grid) return e->fail(PAL_ERR_INVALID, "NULL grid");
  if (!finite3(grid->lo) || !finite3(grid->hi)) return e->fail(PAL_ERR_INVALID, "a grid coordinate is not finite");
  int64_t cells = 1;
  for (int a = 0; a < 3; ++a) {
    if (grid->count[a] < 1) return e->fail(PAL_ERR_INVALID, "grid count[%d] = %d: need at least one cell per axis", a, grid->count[a]);
    if (!(grid->hi[a] > grid->lo[a])) return e->fail(PAL_ERR_INVALID, "grid hi[%d] must be above lo[%d]", a, a);
  }
  for (int a = 0; a < 3; ++a) {
    if (grid->count[a] > kSrpMaxCount) return e->fail(PAL_ERR_UNSUPPORTED, "grid count[%d] = %d exceeds %d", a, grid->count[a], kSrpMaxCount);
    cells *= grid->count[a];
  }
  if (cells > kSrpMaxCells) return e->fail(PAL_ERR_UNSUPPORTED, "a grid of %lld cells exceeds 2^24", (long long)cells);
  *G = int(cells);
  return PAL_OK;
}

static void grid_args(const pal_srp_grid* grid, double (&lo)[3], double (&step)[3]) {
  for (int a = 0; a < 3; ++a) {
    lo[a] = grid->lo[a];
    step[a] = srp_step(grid->lo[a], grid->hi[a], grid->count[a]);
  }
}

int Engine::srp_strips_check(int B, int M, int L, int T, int W) {
  if (B < 1 || M < 2 || L < 1) return fail(PAL_ERR_INVALID, "need B >= 1, M >= 2, L >= 1 (got %d, %d, %d)", B, M, L);
  if (T < 0) return fail(PAL_ERR_INVALID, "strip half-width T = %d is negative", T);
  if (W < 0 || W > kSrpMaxSmooth) return fail(PAL_ERR_INVALID, "smoothing half-width W = %d outside 0..%d", W, kSrpMaxSmooth);
  if (int64_t(T) + W > int64_t(L) - 1) return fail(PAL_ERR_INVALID, "T + W = %lld exceeds L - 1 = %d", (long long)(int64_t(T) + W), L - 1);
  return PAL_OK;
}

int Engine::srp_strips_rows(const double* d_rows, int64_t nrows, int L, int T, int W, double* d_strips) {
  SrpStripArgs a{d_rows, d_strips, nrows * int64_t(2 * T + 1), 2 * L - 1, T, W};
  const int64_t blocks = (a.total + kSrpThreads - 1) / kSrpThreads;
  if (blocks > INT32_MAX) return fail(PAL_ERR_UNSUPPORTED, "too many strip samples in one slice");
  ProfScope ps(this, "k_srp_strips");
  k_srp_strips<<<dim3(unsigned(blocks)), dim3(kSrpThreads), 0, stream>>>(a);
  return check(hipGetLastError(), "k_srp_strips");
}

int Engine::srp_peaks_check(int B, const pal_srp_grid* grid, int K, int R) {
  if (B < 1) return fail(PAL_ERR_INVALID, "need B >= 1");
  if (K < 1 || K > kSrpMaxPeaks) return fail(PAL_ERR_INVALID, "K = %d outside 1..%d", K, kSrpMaxPeaks);
  if (R < 1 || R > kSrpMaxRadius) return fail(PAL_ERR_INVALID, "R = %d outside 1..%d", R, kSrpMaxRadius);
  int G = 0;
  return grid_check(this, grid, &G);
}

int Engine::srp_map_check(int B, int M, int T, const double* mics, double fs, double c, const pal_srp_grid* grid, int K, int R,
                          bool any_output, bool peaks_out) {
  if (B < 1 || M < 2) return fail(PAL_ERR_INVALID, "need B >= 1, M >= 2 (got %d, %d)", B, M);
  if (T < 0) return fail(PAL_ERR_INVALID, "strip half-width T = %d is negative", T);
  if (!mics) return fail(PAL_ERR_INVALID, "NULL buffer");
  if (!(fs > 0) || !std::isfinite(fs) || !(c > 0) || !std::isfinite(c)) return fail(PAL_ERR_INVALID, "fs and c must be positive and finite");
  if (K < 0 || K > kSrpMaxPeaks) return fail(PAL_ERR_INVALID, "K = %d outside 0..%d", K, kSrpMaxPeaks);
  if (K > 0 && (R < 1 || R > kSrpMaxRadius)) return fail(PAL_ERR_INVALID, "R = %d outside 1..%d", R, kSrpMaxRadius);
  if (!any_output) return fail(PAL_ERR_INVALID, "no output requested");
  if (peaks_out && K == 0) return fail(PAL_ERR_INVALID, "peaks need K >= 1");
  for (int i = 0; i < 3 * M; ++i)
    if (!std::isfinite(mics[i])) return fail(PAL_ERR_INVALID, "a microphone coordinate is not finite");
  int G = 0;
  PAL_TRY(grid_check(this, grid, &G));
  if (int64_t(M) > 4096) return fail(PAL_ERR_UNSUPPORTED, "more than 4096 microphones");
  if (int64_t(B) * ((G + kSrpThreads - 1) / kSrpThreads) > INT32_MAX) return fail(PAL_ERR_UNSUPPORTED, "too many frames x cells");
  return PAL_OK;
}

// scratch of the map and the peaks: [mics | clip counters | marks | map]
struct SrpCarve {
  size_t o_mics, o_clip, o_marks, o_map, bytes;
  SrpCarve(int B, int M, int G, bool marks, bool map) {
    Carve c;
    o_mics = c.take(size_t(3) * size_t(M) * sizeof(double));
    o_clip = c.take(size_t(B) * sizeof(unsigned long long));
    o_marks = c.take(marks ? size_t(B) * size_t(G) : 0);
    o_map = c.take(map ? size_t(B) * size_t(G) * sizeof(double) : 0);
    bytes = c.off;
  }
};

static int launch_peaks(Engine* e, const double* d_power, int B, const pal_srp_grid* grid, int G, int K, int R, unsigned char* marks,
                        pal_srp_peak* d_peaks, pal_srp_frame* d_summary, const unsigned long long* d_clipped) {
  SrpPeakArgs a{};
  a.power = d_power;
  a.marks = marks;
  a.peaks = d_peaks;
  a.summary = d_summary;
  a.clipped = d_clipped;
  grid_args(grid, a.lo, a.step);
  a.nx = grid->count[0];
  a.ny = grid->count[1];
  a.nz = grid->count[2];
  a.G = G;
  a.K = K;
  a.R = R;
  ProfScope ps(e, "k_srp_peaks");
  k_srp_peaks<<<dim3(unsigned(B)), dim3(kSrpPeakThreads), 0, e->stream>>>(a);
  return e->check(hipGetLastError(), "k_srp_peaks");
}

int Engine::srp_peaks_dev(const double* d_power, int B, const pal_srp_grid* grid, int K, int R, pal_srp_peak* d_peaks, pal_srp_frame* d_summary) {
  PAL_TRY(srp_peaks_check(B, grid, K, R));
  if (!d_power || !d_peaks) return fail(PAL_ERR_INVALID, "NULL buffer");
  int G = 0;
  PAL_TRY(grid_check(this, grid, &G));
  const SrpCarve c(B, 2, G, true, false);
  char* base = nullptr;
  PAL_TRY(scratch(kWsSrp, c.bytes, &base));
  return launch_peaks(this, d_power, B, grid, G, K, R, reinterpret_cast<unsigned char*>(base + c.o_marks), d_peaks, d_summary, nullptr);
}

int Engine::srp_map_dev(const double* d_strips, int B, int M, int T, const double* mics, double fs, double c, const pal_srp_grid* grid,
                        const double* d_pair_weights, int K, int R, double* d_power, pal_srp_peak* d_peaks, pal_srp_frame* d_summary) {
  PAL_TRY(srp_map_check(B, M, T, mics, fs, c, grid, K, R, d_power || d_peaks || d_summary, d_peaks != nullptr));
  if (!d_strips) return fail(PAL_ERR_INVALID, "NULL buffer");
  int G = 0;
  PAL_TRY(grid_check(this, grid, &G));
  const bool want_peaks = K > 0 && (d_peaks || d_summary);
  const SrpCarve cv(B, M, G, want_peaks, d_power == nullptr);
  char* base = nullptr;
  PAL_TRY(scratch(kWsSrp, cv.bytes, &base));
  // `mics` is host memory: the copy has left it when this returns
  PAL_HIP(hipMemcpyAsync(base + cv.o_mics, mics, size_t(3) * size_t(M) * sizeof(double), hipMemcpyHostToDevice, stream));
  PAL_HIP(hipStreamSynchronize(stream));
  PAL_HIP(hipMemsetAsync(base + cv.o_clip, 0, size_t(B) * sizeof(unsigned long long), stream));
  SrpMapArgs a{};
  a.strips = d_strips;
  a.weights = d_pair_weights;
  a.mics = reinterpret_cast<const double*>(base + cv.o_mics);
  a.power = d_power ? d_power : reinterpret_cast<double*>(base + cv.o_map);
  a.clipped = reinterpret_cast<unsigned long long*>(base + cv.o_clip);
  grid_args(grid, a.lo, a.step);
  a.fs = fs;
  a.c = c;
  a.inv_c = 1.0 / c;
  a.ny = grid->count[1];
  a.nz = grid->count[2];
  a.G = G;
  a.M = M;
  a.P = M * (M - 1) / 2;
  a.T = T;
  a.tiles = (M + kPairTile - 1) / kPairTile;
  a.blocks = (G + kSrpThreads - 1) / kSrpThreads;
  {
    ProfScope ps(this, "k_srp_map");
    k_srp_map<<<dim3(unsigned(B) * unsigned(a.blocks)), dim3(kSrpThreads), 0, stream>>>(a);
  }
  PAL_HIP(hipGetLastError());
  if (!d_peaks && !d_summary) return PAL_OK;
  return launch_peaks(this, a.power, B, grid, G, want_peaks ? K : 0, R, reinterpret_cast<unsigned char*>(base + cv.o_marks), d_peaks, d_summary,
                      a.clipped);
}

int Engine::srp_zoom_check(int B, int M, int T, const double* mics, double fs, double c, int K, const double* half0, int Z, int levels) {
  if (B < 1 || M < 2) return fail(PAL_ERR_INVALID, "need B >= 1, M >= 2 (got %d, %d)", B, M);
  if (T < 1) return fail(PAL_ERR_INVALID, "strip half-width T = %d: the zoom reads two neighbouring samples, need T >= 1", T);
  if (!mics || !half0) return fail(PAL_ERR_INVALID, "NULL buffer");
  if (!(fs > 0) || !std::isfinite(fs) || !(c > 0) || !std::isfinite(c)) return fail(PAL_ERR_INVALID, "fs and c must be positive and finite");
  if (K < 1 || K > kSrpMaxPeaks) return fail(PAL_ERR_INVALID, "K = %d outside 1..%d", K, kSrpMaxPeaks);
  if (Z < 2 || Z > kSrpMaxZoomCells) return fail(PAL_ERR_INVALID, "Z = %d outside 2..%d", Z, kSrpMaxZoomCells);
  if (levels < 1 || levels > kSrpMaxZoomLevels) return fail(PAL_ERR_INVALID, "levels = %d outside 1..%d", levels, kSrpMaxZoomLevels);
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(half0[a]) || !(half0[a] > 0)) return fail(PAL_ERR_INVALID, "half0[%d] must be finite and positive", a);
  for (int i = 0; i < 3 * M; ++i)
    if (!std::isfinite(mics[i])) return fail(PAL_ERR_INVALID, "a microphone coordinate is not finite");
  if (int64_t(M) > 4096) return fail(PAL_ERR_UNSUPPORTED, "more than 4096 microphones");
  if (int64_t(B) * K > INT32_MAX) return fail(PAL_ERR_UNSUPPORTED, "too many frames x seeds");
  return PAL_OK;
}

int Engine::srp_zoom_dev(const double* d_strips, int B, int M, int T, const double* mics, double fs, double c, const double* d_pair_weights,
                         const pal_srp_peak* d_seeds, int K, const double* half0, int Z, int levels, pal_srp_zoom_record* d_out) {
  PAL_TRY(srp_zoom_check(B, M, T, mics, fs, c, K, half0, Z, levels));
  if (!d_strips || !d_seeds || !d_out) return fail(PAL_ERR_INVALID, "NULL buffer");
  const SrpCarve cv(B, M, 0, false, false);
  char* base = nullptr;
  PAL_TRY(scratch(kWsSrp, cv.bytes, &base));
  // `mics` is host memory: the copy has left it when this returns
  PAL_HIP(hipMemcpyAsync(base + cv.o_mics, mics, size_t(3) * size_t(M) * sizeof(double), hipMemcpyHostToDevice, stream));
  PAL_HIP(hipStreamSynchronize(stream));
  SrpZoomArgs a{};
  a.strips = d_strips;
  a.weights = d_pair_weights;
  a.mics = reinterpret_cast<const double*>(base + cv.o_mics);
  a.seeds = d_seeds;
  a.out = d_out;
  for (int ax = 0; ax < 3; ++ax) a.half0[ax] = half0[ax];
  a.fs = fs;
  a.c = c;
  a.M = M;
  a.P = M * (M - 1) / 2;
  a.T = T;
  a.tiles = (M + kPairTile - 1) / kPairTile;
  a.K = K;
  a.Z = Z;
  a.levels = levels;
  {
    ProfScope ps(this, "k_srp_zoom");
    k_srp_zoom<<<dim3(unsigned(B) * unsigned(K)), dim3(kSrpThreads), 0, stream>>>(a);
  }
  return check(hipGetLastError(), "k_srp_zoom");
}

}  // namespace pal
