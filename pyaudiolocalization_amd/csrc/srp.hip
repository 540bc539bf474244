// srp.hip - steered-response power (SRP-PHAT) from all-pairs GCC-PHAT rows: the lag strips, the map over a box of points with its peaks
// and zoom, and the direction map - far-field azimuth / elevation power - with its peaks and its zoom on the sphere
// (pal_gcc_phat_all_pairs_strips*, pal_srp_map*, pal_srp_peaks*, pal_srp_zoom*, pal_srp_doa*, pal_srp_doa_peaks*, pal_srp_doa_zoom*;
// specification: pyaudiolocalization_amd/srp.py; arithmetic: srp_math.h).  Built with -ffp-contract=off.
//
//   k_srp_strips     one lane per output sample of strips[rows][2T+1]: the 2W+1 neighbours of the row around the sample's lag, weighted
//                    by the triangle and added in the specification's order.  It runs behind a frame slice of the pair pipeline, whose
//                    rows [slice pairs][2L-1] sit in engine scratch (pal_api.hip: strips_dev; frames go through in slices whose rows
//                    stay under about 1 GiB, never less than one frame - one frame of 64 microphones and L = 44 100 alone is 1.4 GB).
//                    A row's samples come from HBM once (the neighbours of one sample are the next lanes' samples: L1 / L2 serve
//                    them), coalesced apart from the wrap at lag 0.
// The four cell kernels put one lane on one point and sum every pair's term there with srp_pair_sum (srp_cells.h): microphones in tiles
// of 16, tile ti's path lengths in the lane's LDS column and tile tj >= ti's in registers, the sum in the fixed order (ti, tj, i, j) -
// the same input gives the same bytes whatever B is, and they are srp.py's.  The term was once a functor returning bool with the value
// as an out-parameter; that shape cost k_srp_map two VGPRs and 64 branches, so each kernel kept a copy of the loop.  The term is now a
// policy object (at, clipped, read) and the caller keeps the branch: the kernels compile as the copies did.  No
// floating-point atomics, no waits between workgroups, no scratch memory.
//   k_srp_map        a workgroup takes 256 consecutive linear indices of one frame (SrpMapBlock): with iz fastest, neighbouring lanes'
//                    lags for one pair differ by a sample or two, so a wavefront's 64 reads of a pair touch a few cache lines of that
//                    pair's strip.  A path length is the distance to the cell, computed once per tile pass, not once per pair:
//                    16 (tiles + tiles (tiles + 1) / 2) square roots per cell against M (M - 1) / 2 lags.  Clipped terms are counted
//                    per lane, added up in LDS and leave with one 64-bit integer atomic per workgroup;
//   k_srp_doa        the same frame over directions g = ia * n_el + ie.  A path length is the negated advance -(u . m) of the plane
//                    wave: three products and two additions, no square root; the direction itself is two products of the host's
//                    (cos, sin) tables, so the device evaluates no sine;
//   k_srp_zoom       one workgroup of 256 per (frame, seed) runs every level of the coarse-to-fine zoom (srp.zoom): a level's Z^3 cells
//                    in chunks of 256, one lane per cell, the strip read at the fractional lag (two samples, blended); the level's
//                    best cell by one block reduction, the next box through LDS (srp_cells.h: srp_zoom_begin, srp_zoom_pick).  No
//                    atomics on global memory;
//   k_srp_doa_zoom   the same for srp.doa_zoom: Z^2 <= 256 cells, so a level is one chunk.  Every lane builds the level's tangent
//                    basis from the centre in LDS (one square root and three divisions per level, no barrier for it);
//   k_srp_peaks, k_srp_doa_peaks
//                    one workgroup of 1024 per frame over the stored map (srp_select.h: srp_peaks_frame): marks the peaks by the
//                    neighbourhood rule - the box's, or the direction grid's with azimuth mod n_az when the grid wraps - one byte per
//                    cell in engine scratch, then K selection passes, each the block maximum - in the order power descending, index
//                    ascending - of the marks behind the previous pass's pick; writes peaks[B][K] and the frame's summary.
#include "engine.h"
#include "srp_cells.h"
#include "srp_select.h"

namespace pal {

static_assert(kSrpMaxSmooth == PAL_SRP_MAX_SMOOTH && kSrpMaxPeaks == PAL_SRP_MAX_PEAKS && kSrpMaxRadius == PAL_SRP_MAX_RADIUS,
              "srp_math.h and pal_hip.h state the same limits");
static_assert(sizeof(pal_srp_grid) == 64 && sizeof(pal_srp_peak) == 40 && sizeof(pal_srp_frame) == 16, "record sizes of pal_hip.h");
static_assert(kSrpMaxZoomCells == PAL_SRP_MAX_ZOOM_CELLS && kSrpMaxZoomLevels == PAL_SRP_MAX_ZOOM_LEVELS, "the zoom's limits");
static_assert(sizeof(pal_srp_zoom_record) == 48 && sizeof(pal_srp_doa_grid) == 16, "record sizes of pal_hip.h");
static_assert(kSrpMaxZoomCells * kSrpMaxZoomCells <= kSrpThreads, "a level of the direction zoom is one chunk");

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

// ---- the maps ----
struct SrpMapArgs {
  SrpCellArgs k;
  double* power;                   // [B][G]
  unsigned long long* clipped;     // [B], zeroed before the launch
  double lo[3], step[3];
  int ny, nz, G, blocks;           // blocks: workgroups per frame
};

__global__ __launch_bounds__(kSrpThreads) void k_srp_map(SrpMapArgs a) {
  __shared__ double column[kPairTile * kSrpThreads];   // d[mic of tile ti][lane]: 32 KiB
  __shared__ int clip_sum;
  const SrpMapBlock blk(a.k, a.G, a.blocks, &clip_sum);
  int ix, iy, iz;
  srp_cell(blk.g, a.ny, a.nz, ix, iy, iz);
  const double x = srp_coord(a.lo[0], a.step[0], ix), y = srp_coord(a.lo[1], a.step[1], iy), z = srp_coord(a.lo[2], a.step[2], iz);
  const double* mics = a.k.mics;
  double acc;
  const int clip = srp_pair_sum(
      a.k.M, a.k.tiles, blk.wt, column, threadIdx.x, acc,
      [&](int m) { return srp_distance(x, y, z, mics[3 * m], mics[3 * m + 1], mics[3 * m + 2]); }, srp_nearest_term(a.k, blk.centre));
  blk.finish(a.power, a.clipped, a.G, acc, clip, &clip_sum);
}

struct SrpDoaArgs {
  SrpCellArgs k;
  const double* az;                // [n_az][2]: cos, sin
  const double* el;                // [n_el][2]
  double* power;                   // [B][G]
  unsigned long long* clipped;     // [B], zeroed before the launch
  int n_el, G, blocks;             // blocks: workgroups per frame
};

__global__ __launch_bounds__(kSrpThreads) void k_srp_doa(SrpDoaArgs a) {
  __shared__ double column[kPairTile * kSrpThreads];   // -a[mic of tile ti][lane]: 32 KiB
  __shared__ int clip_sum;
  const SrpMapBlock blk(a.k, a.G, a.blocks, &clip_sum);
  int ia, ie;
  srp_doa_cell(blk.g, a.n_el, ia, ie);
  double ux, uy, uz;
  srp_doa_direction(a.az[2 * ia], a.az[2 * ia + 1], a.el[2 * ie], a.el[2 * ie + 1], ux, uy, uz);
  const double* mics = a.k.mics;
  double acc;
  const int clip = srp_pair_sum(
      a.k.M, a.k.tiles, blk.wt, column, threadIdx.x, acc,
      [&](int m) { return -srp_doa_advance(ux, uy, uz, mics[3 * m], mics[3 * m + 1], mics[3 * m + 2]); }, srp_nearest_term(a.k, blk.centre));
  blk.finish(a.power, a.clipped, a.G, acc, clip, &clip_sum);
}

// ---- the peaks ----
struct SrpPeakArgs {
  SrpPeakIo io;
  double lo[3], step[3];
  int nx, ny, nz, R;
};

__global__ __launch_bounds__(kSrpPeakThreads) void k_srp_peaks(SrpPeakArgs a) {
  srp_peaks_frame(
      a.io,
      [&](const double* power, int g) {
        int ix, iy, iz;
        srp_cell(g, a.ny, a.nz, ix, iy, iz);
        return srp_is_peak(power, a.nx, a.ny, a.nz, ix, iy, iz, a.R);
      },
      [&](int g, pal_srp_peak& rec) {
        int ix, iy, iz;
        srp_cell(g, a.ny, a.nz, ix, iy, iz);
        rec.x = srp_coord(a.lo[0], a.step[0], ix);
        rec.y = srp_coord(a.lo[1], a.step[1], iy);
        rec.z = srp_coord(a.lo[2], a.step[2], iz);
      });
}

struct SrpDoaPeakArgs {
  SrpPeakIo io;
  const double* az;                     // [n_az][2]
  const double* el;                     // [n_el][2]
  int n_az, n_el, wrap, R;
};

__global__ __launch_bounds__(kSrpPeakThreads) void k_srp_doa_peaks(SrpDoaPeakArgs a) {
  srp_peaks_frame(
      a.io,
      [&](const double* power, int g) {
        int ia, ie;
        srp_doa_cell(g, a.n_el, ia, ie);
        return srp_doa_is_peak(power, a.n_az, a.n_el, a.wrap, ia, ie, a.R);
      },
      [&](int g, pal_srp_peak& rec) {       // a record's x, y, z is the cell's direction
        int ia, ie;
        srp_doa_cell(g, a.n_el, ia, ie);
        srp_doa_direction(a.az[2 * ia], a.az[2 * ia + 1], a.el[2 * ie], a.el[2 * ie + 1], rec.x, rec.y, rec.z);
      });
}

// ---- the zooms: one workgroup per (frame, seed) runs every level.  The level's centre sits in LDS (SrpZoomLds), its half-extent beside
// it; every lane computes the same cells from them and keeps its best (power, index) by srp_before with NaN never entered; srp_zoom_pick
// takes the level's best and thread 0 writes the next level's centre and half-extent.  The stop flag comes back from LDS behind a
// barrier, so the whole workgroup leaves together.  Two barriers per level.  The record belongs to this workgroup: no global atomics.
struct SrpZoomArgs {
  SrpCellArgs k;
  const pal_srp_peak* seeds;       // [B][K]
  pal_srp_zoom_record* out;        // [B][K]
  double half0[3];                 // the direction zoom's one half-extent, in tangent units, is half0[0]
  int K, Z, levels;
};

// a level is a box of Z^3 cells around the centre: they go through in chunks of 256, one lane per cell, and the best cell's centre and
// size are the next box's
__global__ __launch_bounds__(kSrpThreads) void k_srp_zoom(SrpZoomArgs a) {
  __shared__ double column[kPairTile * kSrpThreads];   // d[mic of tile ti][lane]: 32 KiB
  __shared__ SrpZoomLds s;
  __shared__ double half[3];
  const int tid = threadIdx.x, b = blockIdx.x / a.K, Z = a.Z, G = Z * Z * Z;
  if (tid == 0)
    for (int ax = 0; ax < 3; ++ax) half[ax] = a.half0[ax];
  pal_srp_zoom_record rec;                          // thread 0's
  const bool absent = srp_zoom_begin(a.seeds, s, rec);   // uniform
  const double* wt = srp_frame_weights(a.k, b);
  const double* mics = a.k.mics;
  const SrpBlendTerm term = srp_blend_term(a.k, srp_frame_centre(a.k, b));
  for (int level = 0; level < a.levels && !absent; ++level) {
    double lo[3], step[3];
    for (int ax = 0; ax < 3; ++ax) {
      double hi;
      srp_zoom_box(s.ctr[ax], half[ax], lo[ax], hi);
      step[ax] = srp_step(lo[ax], hi, Z);
    }
    double my_p = 0.0;
    int my_g = -1, clip = 0;
    for (int g0 = tid; g0 - tid < G; g0 += kSrpThreads) {   // every lane runs every chunk
      const bool active = g0 < G;
      const int g = active ? g0 : G - 1;            // a lane past Z^3 computes the last cell and takes no part in the reduction
      int ix, iy, iz;
      srp_cell(g, Z, Z, ix, iy, iz);
      const double x = srp_coord(lo[0], step[0], ix), y = srp_coord(lo[1], step[1], iy), z = srp_coord(lo[2], step[2], iz);
      double p;
      const int c = srp_pair_sum(
          a.k.M, a.k.tiles, wt, column, tid, p,
          [&](int m) { return srp_distance(x, y, z, mics[3 * m], mics[3 * m + 1], mics[3 * m + 2]); }, term);
      if (active) {
        clip += c;
        if (p == p && (my_g < 0 || srp_before(p, g, my_p, my_g))) { my_p = p; my_g = g; }
      }
    }
    const bool stop = srp_zoom_pick(s, my_p, my_g, clip, level, rec, [&](int best, double* c3) {
      int ix, iy, iz;
      srp_cell(best, Z, Z, ix, iy, iz);
      const int cell[3] = {ix, iy, iz};
      for (int ax = 0; ax < 3; ++ax) {
        c3[ax] = srp_coord(lo[ax], step[ax], cell[ax]);
        half[ax] = step[ax];                        // srp_zoom_next_half(lo, hi, Z): one cell of this level
      }
    });
    if (stop) break;                                // uniform
  }
  if (tid == 0) a.out[blockIdx.x] = rec;
}

// a level is Z^2 cells of the centre's tangent plane: lane tid takes cell tid = i * Z + j (a lane past Z^2 computes the last cell and
// takes no part in the reduction), and the best cell's point is the next centre
__global__ __launch_bounds__(kSrpThreads) void k_srp_doa_zoom(SrpZoomArgs a) {
  __shared__ double column[kPairTile * kSrpThreads];   // -a[mic of tile ti][lane]: 32 KiB
  __shared__ SrpZoomLds s;
  __shared__ double half;
  const int tid = threadIdx.x, b = blockIdx.x / a.K, Z = a.Z, G = Z * Z;
  if (tid == 0) half = a.half0[0];
  pal_srp_zoom_record rec;                          // thread 0's
  const bool absent = srp_zoom_begin(a.seeds, s, rec);   // uniform
  const double* wt = srp_frame_weights(a.k, b);
  const double* mics = a.k.mics;
  const SrpBlendTerm term = srp_blend_term(a.k, srp_frame_centre(a.k, b));
  const bool active = tid < G;
  const int g = active ? tid : G - 1;
  for (int level = 0; level < a.levels && !absent; ++level) {
    const double u[3] = {s.ctr[0], s.ctr[1], s.ctr[2]}, h = half;
    double e1[3], e2[3], v[3];
    srp_doa_basis(u, e1, e2);
    const double step = srp_step(-h, h, Z);
    srp_doa_point(u, e1, e2, srp_coord(-h, step, g / Z), srp_coord(-h, step, g % Z), v);
    double my_p;
    const int clip = srp_pair_sum(
        a.k.M, a.k.tiles, wt, column, tid, my_p,
        [&](int m) { return -srp_doa_advance(v[0], v[1], v[2], mics[3 * m], mics[3 * m + 1], mics[3 * m + 2]); }, term);
    const int my_g = active && my_p == my_p ? g : -1;   // NaN never enters
    const bool stop = srp_zoom_pick(s, my_p, my_g, active ? clip : 0, level, rec, [&](int best, double* c3) {
      srp_doa_point(u, e1, e2, srp_coord(-h, step, best / Z), srp_coord(-h, step, best % Z), c3);   // the same bits as the cell's lane
      half = srp_zoom_next_half(-h, h, Z);
    });
    if (stop) break;                                // uniform
  }
  if (tid == 0) a.out[blockIdx.x] = rec;
}

// ---- host side ----

static bool finite3(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// the box grid's own checks -> G
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

// the direction grid's and its tables' own checks -> G
static int doa_grid_check(Engine* e, const pal_srp_doa_grid* grid, const double* az, const double* el, int* G) {
  if (!grid || !az || !el) return e->fail(PAL_ERR_INVALID, "NULL grid or direction table");
  if (grid->n_az < 1 || grid->n_el < 1)
    return e->fail(PAL_ERR_INVALID, "a direction grid of %d x %d: need at least one azimuth and one elevation", grid->n_az, grid->n_el);
  if (grid->n_az > kSrpMaxDoaCount || grid->n_el > kSrpMaxDoaCount)
    return e->fail(PAL_ERR_UNSUPPORTED, "a direction grid of %d x %d exceeds %d per axis", grid->n_az, grid->n_el, kSrpMaxDoaCount);
  for (int i = 0; i < 2 * grid->n_az; ++i)
    if (!std::isfinite(az[i])) return e->fail(PAL_ERR_INVALID, "an azimuth table entry is not finite");
  for (int i = 0; i < 2 * grid->n_el; ++i)
    if (!std::isfinite(el[i])) return e->fail(PAL_ERR_INVALID, "an elevation table entry is not finite");
  *G = grid->n_az * grid->n_el;
  return PAL_OK;
}

static void grid_args(const pal_srp_grid* grid, double (&lo)[3], double (&step)[3]) {
  for (int a = 0; a < 3; ++a) {
    lo[a] = grid->lo[a];
    step[a] = srp_step(grid->lo[a], grid->hi[a], grid->count[a]);
  }
}

// What the maps and the zooms check alike, the cheap checks first.  A zoom has T >= 1 (it reads two neighbouring samples) and K >= 1,
// no radius and no choice of outputs.
static int cells_check(Engine* e, int B, int M, int T, bool zoom, const double* mics, double fs, double c, int K, int R, bool any_output,
                       bool peaks_out) {
  if (B < 1 || M < 2) return e->fail(PAL_ERR_INVALID, "need B >= 1, M >= 2 (got %d, %d)", B, M);
  if (zoom && T < 1) return e->fail(PAL_ERR_INVALID, "strip half-width T = %d: the zoom reads two neighbouring samples, need T >= 1", T);
  if (T < 0) return e->fail(PAL_ERR_INVALID, "strip half-width T = %d is negative", T);
  if (!mics) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  if (!(fs > 0) || !std::isfinite(fs) || !(c > 0) || !std::isfinite(c)) return e->fail(PAL_ERR_INVALID, "fs and c must be positive and finite");
  const int k_min = zoom ? 1 : 0;
  if (K < k_min || K > kSrpMaxPeaks) return e->fail(PAL_ERR_INVALID, "K = %d outside %d..%d", K, k_min, kSrpMaxPeaks);
  if (!zoom && K > 0 && (R < 1 || R > kSrpMaxRadius)) return e->fail(PAL_ERR_INVALID, "R = %d outside 1..%d", R, kSrpMaxRadius);
  if (!any_output) return e->fail(PAL_ERR_INVALID, "no output requested");
  if (peaks_out && K == 0) return e->fail(PAL_ERR_INVALID, "peaks need K >= 1");
  if (int64_t(M) > 4096) return e->fail(PAL_ERR_UNSUPPORTED, "more than 4096 microphones");
  for (int i = 0; i < 3 * M; ++i)
    if (!std::isfinite(mics[i])) return e->fail(PAL_ERR_INVALID, "a microphone coordinate is not finite");
  return PAL_OK;
}

static int peaks_check(Engine* e, int B, int K, int R) {
  if (B < 1) return e->fail(PAL_ERR_INVALID, "need B >= 1");
  if (K < 1 || K > kSrpMaxPeaks) return e->fail(PAL_ERR_INVALID, "K = %d outside 1..%d", K, kSrpMaxPeaks);
  if (R < 1 || R > kSrpMaxRadius) return e->fail(PAL_ERR_INVALID, "R = %d outside 1..%d", R, kSrpMaxRadius);
  return PAL_OK;
}

static int map_size_check(Engine* e, int B, int G) {
  if (int64_t(B) * ((G + kSrpThreads - 1) / kSrpThreads) > INT32_MAX) return e->fail(PAL_ERR_UNSUPPORTED, "too many frames x cells");
  return PAL_OK;
}

int Engine::srp_strips_check(int B, int M, int L, int T, int W) {
  if (B < 1 || M < 2 || L < 1) return fail(PAL_ERR_INVALID, "need B >= 1, M >= 2, L >= 1 (got %d, %d, %d)", B, M, L);
  if (T < 0) return fail(PAL_ERR_INVALID, "strip half-width T = %d is negative", T);
  if (W < 0 || W > kSrpMaxSmooth) return fail(PAL_ERR_INVALID, "smoothing half-width W = %d outside 0..%d", W, kSrpMaxSmooth);
  if (int64_t(T) + W > int64_t(L) - 1) return fail(PAL_ERR_INVALID, "T + W = %lld exceeds L - 1 = %d", (long long)(int64_t(T) + W), L - 1);
  return PAL_OK;
}

int Engine::srp_peaks_check(int B, const pal_srp_grid* grid, int K, int R) {
  PAL_TRY(peaks_check(this, B, K, R));
  int G = 0;
  return grid_check(this, grid, &G);
}

int Engine::srp_doa_peaks_check(int B, const pal_srp_doa_grid* grid, const double* az, const double* el, int K, int R) {
  PAL_TRY(peaks_check(this, B, K, R));
  int G = 0;
  return doa_grid_check(this, grid, az, el, &G);
}

int Engine::srp_map_check(int B, int M, int T, const double* mics, double fs, double c, const pal_srp_grid* grid, int K, int R,
                          bool any_output, bool peaks_out) {
  PAL_TRY(cells_check(this, B, M, T, false, mics, fs, c, K, R, any_output, peaks_out));
  int G = 0;
  PAL_TRY(grid_check(this, grid, &G));
  return map_size_check(this, B, G);
}

int Engine::srp_doa_check(int B, int M, int T, const double* mics, double fs, double c, const pal_srp_doa_grid* grid, const double* az,
                          const double* el, int K, int R, bool any_output, bool peaks_out) {
  PAL_TRY(cells_check(this, B, M, T, false, mics, fs, c, K, R, any_output, peaks_out));
  int G = 0;
  PAL_TRY(doa_grid_check(this, grid, az, el, &G));
  return map_size_check(this, B, G);
}

int Engine::srp_zoom_check(int B, int M, int T, const double* mics, double fs, double c, int K, const double* half0, int Z, int levels) {
  PAL_TRY(cells_check(this, B, M, T, true, mics, fs, c, K, 0, true, false));
  if (!half0) return fail(PAL_ERR_INVALID, "NULL buffer");
  if (Z < 2 || Z > kSrpMaxZoomCells) return fail(PAL_ERR_INVALID, "Z = %d outside 2..%d", Z, kSrpMaxZoomCells);
  if (levels < 1 || levels > kSrpMaxZoomLevels) return fail(PAL_ERR_INVALID, "levels = %d outside 1..%d", levels, kSrpMaxZoomLevels);
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(half0[a]) || !(half0[a] > 0)) return fail(PAL_ERR_INVALID, "half0[%d] must be finite and positive", a);
  if (int64_t(B) * K > INT32_MAX) return fail(PAL_ERR_UNSUPPORTED, "too many frames x seeds");
  return PAL_OK;
}

int Engine::srp_doa_zoom_check(int B, int M, int T, const double* mics, double fs, double c, int K, double half0, int Z, int levels) {
  const double h3[3] = {half0, half0, half0};       // one half-extent, in tangent units: the box zoom's checks on it and on all else
  return srp_zoom_check(B, M, T, mics, fs, c, K, h3, Z, levels);
}

// scratch of every call below: [mics | az | el | clip counters | marks | map]; a piece the call does not use is empty
struct SrpCarve {
  size_t o_mics, o_az, o_el, o_clip, o_marks, o_map, bytes;
  SrpCarve(int B, int M, int n_az, int n_el, int G, bool marks, bool map) {
    Carve c;
    o_mics = c.take(size_t(3) * size_t(M) * sizeof(double));
    o_az = c.take(size_t(2) * size_t(n_az) * sizeof(double));
    o_el = c.take(size_t(2) * size_t(n_el) * sizeof(double));
    o_clip = c.take(size_t(B) * sizeof(unsigned long long));
    o_marks = c.take(marks ? size_t(B) * size_t(G) : 0);
    o_map = c.take(map ? size_t(B) * size_t(G) * sizeof(double) : 0);
    bytes = c.off;
  }
};

// the engine's SRP scratch carved by `cv`, with the host tables in it (a count of 0: no such table): they have left host memory when
// this returns
static int srp_scratch(Engine* e, const SrpCarve& cv, const double* mics, int M, const double* az, int n_az, const double* el, int n_el,
                       char** base) {
  PAL_TRY(e->scratch(kWsSrp, cv.bytes, base));
  const auto up = [&](size_t at, const double* src, size_t count) {
    if (!count) return int(PAL_OK);
    return e->check(hipMemcpyAsync(*base + at, src, count * sizeof(double), hipMemcpyHostToDevice, e->stream), "table upload");
  };
  PAL_TRY(up(cv.o_mics, mics, size_t(3) * size_t(M)));
  PAL_TRY(up(cv.o_az, az, size_t(2) * size_t(n_az)));
  PAL_TRY(up(cv.o_el, el, size_t(2) * size_t(n_el)));
  return e->check(hipStreamSynchronize(e->stream), "table upload");
}

static SrpCellArgs cell_args(const double* d_strips, const double* d_pair_weights, const char* base, const SrpCarve& cv, int M, int T,
                             double fs, double c) {
  SrpCellArgs k{};
  k.strips = d_strips;
  k.weights = d_pair_weights;
  k.mics = reinterpret_cast<const double*>(base + cv.o_mics);
  k.fs = fs;
  k.c = c;
  k.inv_c = 1.0 / c;
  k.M = M;
  k.P = M * (M - 1) / 2;
  k.T = T;
  k.tiles = (M + kPairTile - 1) / kPairTile;
  return k;
}

// a peak kernel over d_power[B][G]; `a` comes with its own fields filled
template <class ARGS>
static int launch_peaks(Engine* e, void (*kernel)(ARGS), const char* name, ARGS& a, const double* d_power, int B, int G, int K, char* base,
                        const SrpCarve& cv, pal_srp_peak* d_peaks, pal_srp_frame* d_summary, const unsigned long long* d_clipped) {
  a.io = SrpPeakIo{d_power, reinterpret_cast<unsigned char*>(base + cv.o_marks), d_peaks, d_summary, d_clipped, G, K};
  ProfScope ps(e, name);
  kernel<<<dim3(unsigned(B)), dim3(kSrpPeakThreads), 0, e->stream>>>(a);
  return e->check(hipGetLastError(), name);
}

static int box_peaks(Engine* e, const double* d_power, int B, const pal_srp_grid* grid, int G, int K, int R, char* base, const SrpCarve& cv,
                     pal_srp_peak* d_peaks, pal_srp_frame* d_summary, const unsigned long long* d_clipped) {
  SrpPeakArgs a{};
  grid_args(grid, a.lo, a.step);
  a.nx = grid->count[0];
  a.ny = grid->count[1];
  a.nz = grid->count[2];
  a.R = R;
  return launch_peaks(e, k_srp_peaks, "k_srp_peaks", a, d_power, B, G, K, base, cv, d_peaks, d_summary, d_clipped);
}

static int doa_peaks(Engine* e, const double* d_power, int B, const pal_srp_doa_grid* grid, int G, int K, int R, char* base,
                     const SrpCarve& cv, pal_srp_peak* d_peaks, pal_srp_frame* d_summary, const unsigned long long* d_clipped) {
  SrpDoaPeakArgs a{};
  a.az = reinterpret_cast<const double*>(base + cv.o_az);
  a.el = reinterpret_cast<const double*>(base + cv.o_el);
  a.n_az = grid->n_az;
  a.n_el = grid->n_el;
  a.wrap = grid->wrap;
  a.R = R;
  return launch_peaks(e, k_srp_doa_peaks, "k_srp_doa_peaks", a, d_power, B, G, K, base, cv, d_peaks, d_summary, d_clipped);
}

int Engine::srp_strips_rows(const double* d_rows, int64_t nrows, int L, int T, int W, double* d_strips) {
  SrpStripArgs a{d_rows, d_strips, nrows * int64_t(2 * T + 1), 2 * L - 1, T, W};
  const int64_t blocks = (a.total + kSrpThreads - 1) / kSrpThreads;
  if (blocks > INT32_MAX) return fail(PAL_ERR_UNSUPPORTED, "too many strip samples in one slice");
  ProfScope ps(this, "k_srp_strips");
  k_srp_strips<<<dim3(unsigned(blocks)), dim3(kSrpThreads), 0, stream>>>(a);
  return check(hipGetLastError(), "k_srp_strips");
}

int Engine::srp_peaks_dev(const double* d_power, int B, const pal_srp_grid* grid, int K, int R, pal_srp_peak* d_peaks, pal_srp_frame* d_summary) {
  PAL_TRY(srp_peaks_check(B, grid, K, R));
  if (!d_power || !d_peaks) return fail(PAL_ERR_INVALID, "NULL buffer");
  int G = 0;
  PAL_TRY(grid_check(this, grid, &G));
  const SrpCarve cv(B, 2, 0, 0, G, true, false);
  char* base = nullptr;
  PAL_TRY(scratch(kWsSrp, cv.bytes, &base));
  return box_peaks(this, d_power, B, grid, G, K, R, base, cv, d_peaks, d_summary, nullptr);
}

int Engine::srp_doa_peaks_dev(const double* d_power, int B, const pal_srp_doa_grid* grid, const double* az, const double* el, int K, int R,
                              pal_srp_peak* d_peaks, pal_srp_frame* d_summary) {
  PAL_TRY(srp_doa_peaks_check(B, grid, az, el, K, R));
  if (!d_power || !d_peaks) return fail(PAL_ERR_INVALID, "NULL buffer");
  const int G = grid->n_az * grid->n_el;
  const SrpCarve cv(B, 0, grid->n_az, grid->n_el, G, true, false);
  char* base = nullptr;
  PAL_TRY(srp_scratch(this, cv, nullptr, 0, az, grid->n_az, el, grid->n_el, &base));
  return doa_peaks(this, d_power, B, grid, G, K, R, base, cv, d_peaks, d_summary, nullptr);
}

int Engine::srp_map_dev(const double* d_strips, int B, int M, int T, const double* mics, double fs, double c, const pal_srp_grid* grid,
                        const double* d_pair_weights, int K, int R, double* d_power, pal_srp_peak* d_peaks, pal_srp_frame* d_summary) {
  PAL_TRY(srp_map_check(B, M, T, mics, fs, c, grid, K, R, d_power || d_peaks || d_summary, d_peaks != nullptr));
  if (!d_strips) return fail(PAL_ERR_INVALID, "NULL buffer");
  int G = 0;
  PAL_TRY(grid_check(this, grid, &G));
  const bool want_peaks = K > 0 && (d_peaks || d_summary);
  const SrpCarve cv(B, M, 0, 0, G, want_peaks, d_power == nullptr);
  char* base = nullptr;
  PAL_TRY(srp_scratch(this, cv, mics, M, nullptr, 0, nullptr, 0, &base));
  PAL_HIP(hipMemsetAsync(base + cv.o_clip, 0, size_t(B) * sizeof(unsigned long long), stream));
  SrpMapArgs a{};
  a.k = cell_args(d_strips, d_pair_weights, base, cv, M, T, fs, c);
  a.power = d_power ? d_power : reinterpret_cast<double*>(base + cv.o_map);
  a.clipped = reinterpret_cast<unsigned long long*>(base + cv.o_clip);
  grid_args(grid, a.lo, a.step);
  a.ny = grid->count[1];
  a.nz = grid->count[2];
  a.G = G;
  a.blocks = (G + kSrpThreads - 1) / kSrpThreads;
  {
    ProfScope ps(this, "k_srp_map");
    k_srp_map<<<dim3(unsigned(B) * unsigned(a.blocks)), dim3(kSrpThreads), 0, stream>>>(a);
  }
  PAL_HIP(hipGetLastError());
  if (!d_peaks && !d_summary) return PAL_OK;
  return box_peaks(this, a.power, B, grid, G, want_peaks ? K : 0, R, base, cv, d_peaks, d_summary, a.clipped);
}

int Engine::srp_doa_dev(const double* d_strips, int B, int M, int T, const double* mics, double fs, double c, const pal_srp_doa_grid* grid,
                        const double* az, const double* el, const double* d_pair_weights, int K, int R, double* d_power,
                        pal_srp_peak* d_peaks, pal_srp_frame* d_summary) {
  PAL_TRY(srp_doa_check(B, M, T, mics, fs, c, grid, az, el, K, R, d_power || d_peaks || d_summary, d_peaks != nullptr));
  if (!d_strips) return fail(PAL_ERR_INVALID, "NULL buffer");
  const int G = grid->n_az * grid->n_el;
  const bool want_peaks = K > 0 && (d_peaks || d_summary);
  const SrpCarve cv(B, M, grid->n_az, grid->n_el, G, want_peaks, d_power == nullptr);
  char* base = nullptr;
  PAL_TRY(srp_scratch(this, cv, mics, M, az, grid->n_az, el, grid->n_el, &base));
  PAL_HIP(hipMemsetAsync(base + cv.o_clip, 0, size_t(B) * sizeof(unsigned long long), stream));
  SrpDoaArgs a{};
  a.k = cell_args(d_strips, d_pair_weights, base, cv, M, T, fs, c);
  a.az = reinterpret_cast<const double*>(base + cv.o_az);
  a.el = reinterpret_cast<const double*>(base + cv.o_el);
  a.power = d_power ? d_power : reinterpret_cast<double*>(base + cv.o_map);
  a.clipped = reinterpret_cast<unsigned long long*>(base + cv.o_clip);
  a.n_el = grid->n_el;
  a.G = G;
  a.blocks = (G + kSrpThreads - 1) / kSrpThreads;
  {
    ProfScope ps(this, "k_srp_doa");
    k_srp_doa<<<dim3(unsigned(B) * unsigned(a.blocks)), dim3(kSrpThreads), 0, stream>>>(a);
  }
  PAL_HIP(hipGetLastError());
  if (!d_peaks && !d_summary) return PAL_OK;
  return doa_peaks(this, a.power, B, grid, G, want_peaks ? K : 0, R, base, cv, d_peaks, d_summary, a.clipped);
}

// both zooms behind their checks: the direction zoom's half-extent arrives as half0[0]
static int zoom_dev(Engine* e, void (*kernel)(SrpZoomArgs), const char* name, const double* d_strips, int B, int M, int T, const double* mics,
                    double fs, double c, const double* d_pair_weights, const pal_srp_peak* d_seeds, int K, const double* half0, int Z,
                    int levels, pal_srp_zoom_record* d_out) {
  if (!d_strips || !d_seeds || !d_out) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  const SrpCarve cv(B, M, 0, 0, 0, false, false);
  char* base = nullptr;
  PAL_TRY(srp_scratch(e, cv, mics, M, nullptr, 0, nullptr, 0, &base));
  SrpZoomArgs a{};
  a.k = cell_args(d_strips, d_pair_weights, base, cv, M, T, fs, c);
  a.seeds = d_seeds;
  a.out = d_out;
  for (int ax = 0; ax < 3; ++ax) a.half0[ax] = half0[ax];
  a.K = K;
  a.Z = Z;
  a.levels = levels;
  {
    ProfScope ps(e, name);
    kernel<<<dim3(unsigned(B) * unsigned(K)), dim3(kSrpThreads), 0, e->stream>>>(a);
  }
  return e->check(hipGetLastError(), name);
}

int Engine::srp_zoom_dev(const double* d_strips, int B, int M, int T, const double* mics, double fs, double c, const double* d_pair_weights,
                         const pal_srp_peak* d_seeds, int K, const double* half0, int Z, int levels, pal_srp_zoom_record* d_out) {
  PAL_TRY(srp_zoom_check(B, M, T, mics, fs, c, K, half0, Z, levels));
  return zoom_dev(this, k_srp_zoom, "k_srp_zoom", d_strips, B, M, T, mics, fs, c, d_pair_weights, d_seeds, K, half0, Z, levels, d_out);
}

int Engine::srp_doa_zoom_dev(const double* d_strips, int B, int M, int T, const double* mics, double fs, double c,
                             const double* d_pair_weights, const pal_srp_peak* d_seeds, int K, double half0, int Z, int levels,
                             pal_srp_zoom_record* d_out) {
  PAL_TRY(srp_doa_zoom_check(B, M, T, mics, fs, c, K, half0, Z, levels));
  const double h3[3] = {half0, half0, half0};
  return zoom_dev(this, k_srp_doa_zoom, "k_srp_doa_zoom", d_strips, B, M, T, mics, fs, c, d_pair_weights, d_seeds, K, h3, Z, levels, d_out);
}

}  // namespace pal
