// srp_cells.h - what the four cell kernels of srp.hip share (k_srp_map, k_srp_zoom, k_srp_doa, k_srp_doa_zoom), each piece once:
//   srp_pair_sum      the power of one point: all pairs' terms in the order of srp.tile_order.  The geometry is a `steer` callable, the
//                     strip read a `term` policy (SrpNearestTerm, SrpBlendTerm).  It reads no threadIdx and includes only srp_math.h
//                     and closure_tiles.h, so it compiles for the host too: tests/host/test_srp_pair_sum.cpp runs it against srp.py;
//   SrpMapBlock       the block frame of the two map kernels: frame and cell from blockIdx, the store, the clip count's way out;
//   SrpZoomLds, srp_zoom_begin, srp_zoom_pick
//                     the level machinery of the two zoom kernels: the record begun from the seed, a level's block reduction with its
//                     clip sum, thread 0's stop-or-advance decision.
// Built with -ffp-contract=off wherever it is used (srp_math.h).
#pragma once
#include "closure_tiles.h"
#include "srp_math.h"

namespace pal {

constexpr int kSrpThreads = 256;         // lanes of a cell kernel's workgroup: one cell each

// what every cell kernel is told about the strips and the array (srp.hip: cell_args)
struct SrpCellArgs {
  const double* strips;            // [B][P][2T+1]
  const double* weights;           // [B][P] or nullptr
  const double* mics;              // [M][3]
  double fs, c, inv_c;
  int M, P, T, tiles;
};

// ---- the two terms.  at(si, sj): where pair (i, j) reads its strip, from the two steers; clipped(at): the term adds nothing and is
// counted; read(p, at): pair p's term, asked only where it is not clipped.  `centre` is strips[frame][0] + T: sample 0 of pair 0 ----

// the maps' term: the strip's sample at the nearest lag
struct SrpNearestTerm {
  const double* centre;
  double fs, c, inv_c;
  int T, width;
  PAL_SRP_HD double at(double si, double sj) const { return srp_lag(si, sj, fs, c, inv_c); }
  PAL_SRP_HD bool clipped(double lag) const { return srp_clipped(lag, T); }
  PAL_SRP_HD double read(int64_t p, double lag) const { return centre[p * int64_t(width) + int(lag)]; }   // signed: the lag may be negative
};

// the zooms' term: the two samples around the fractional lag, blended (srp_zoom_term's pieces)
struct SrpBlendTerm {
  const double* centre;
  double fs, c;
  int T, width;
  PAL_SRP_HD double at(double si, double sj) const { return srp_zoom_quotient(si, sj, fs, c); }
  PAL_SRP_HD bool clipped(double q) const { return srp_zoom_clipped(srp_zoom_floor(q), T); }
  PAL_SRP_HD double read(int64_t p, double q) const { return srp_zoom_read(centre + p * int64_t(width), q); }
};

// The power of one point.  steer(m) is microphone m's path length up to a constant: its distance from the point (near field) or the
// negated advance of the plane wave (far field; negation is exact, so (-a_j) - (-a_i) has the bits of a_i - a_j).  Microphones go
// through in tiles of kPairTile: tile ti's 16 steers sit in this lane's column of `column` ([kPairTile][kSrpThreads], entry
// r * kSrpThreads + tid - a lane reads only what it wrote, so there is no barrier), tile tj >= ti's 16 in registers with the loop over
// them unrolled; a steer is computed once per tile pass, not once per pair.  The sum runs in the fixed order (ti, tj, i, j), one rounded
// product (the weight's) and one rounded addition per term.  wt: this frame's pair weights or nullptr.  -> clipped terms
template <class STEER, class TERM>
PAL_SRP_HD int srp_pair_sum(int M, int tiles, const double* wt, double* column, int tid, double& power, STEER steer, TERM term) {
  double acc = 0.0;
  int clip = 0;
  for (int ti = 0; ti < tiles; ++ti) {
    for (int r = 0; r < kPairTile; ++r) {
      const int i = ti * kPairTile + r;
      if (i < M) column[r * kSrpThreads + tid] = steer(i);
    }
    for (int tj = ti; tj < tiles; ++tj) {
      double s_j[kPairTile];
#pragma unroll
      for (int r = 0; r < kPairTile; ++r) {
        const int j = tj * kPairTile + r;
        s_j[r] = j < M ? steer(j) : 0.0;
      }
      for (int r = 0; r < kPairTile; ++r) {
        const int i = ti * kPairTile + r;
        if (i >= M - 1) break;
        const double s_i = column[r * kSrpThreads + tid];
        const int64_t row0 = pair_row(int64_t(i), int64_t(M));
#pragma unroll
        for (int q = 0; q < kPairTile; ++q) {
          const int j = tj * kPairTile + q;
          if (j > i && j < M) {                    // uniform over the workgroup
            const double at = term.at(s_i, s_j[q]);
            if (term.clipped(at)) {
              ++clip;
            } else {
              double v = term.read(row0 + j, at);
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

}  // namespace pal

#if defined(__HIPCC__)
#include "engine.h"
#include "wave_reduce.h"

namespace pal {

__device__ __forceinline__ SrpNearestTerm srp_nearest_term(const SrpCellArgs& k, const double* centre) {
  return SrpNearestTerm{centre, k.fs, k.c, k.inv_c, k.T, 2 * k.T + 1};
}
__device__ __forceinline__ SrpBlendTerm srp_blend_term(const SrpCellArgs& k, const double* centre) {
  return SrpBlendTerm{centre, k.fs, k.c, k.T, 2 * k.T + 1};
}
// frame b's strips at the centre of pair 0, and its weights or nullptr
__device__ __forceinline__ const double* srp_frame_centre(const SrpCellArgs& k, int b) {
  return k.strips + size_t(b) * size_t(k.P) * size_t(2 * k.T + 1) + k.T;
}
__device__ __forceinline__ const double* srp_frame_weights(const SrpCellArgs& k, int b) {
  return k.weights ? k.weights + size_t(b) * size_t(k.P) : nullptr;
}

// ---- the block frame of a map kernel: a workgroup takes 256 consecutive cells of one frame, `blocks` workgroups per frame ----
struct SrpMapBlock {
  int b, g;                        // frame; this lane's cell
  bool active;                     // a lane past the grid computes the last cell and writes nothing
  const double* centre;            // srp_frame_centre, srp_frame_weights
  const double* wt;

  // clip_sum: one int of LDS; the first barrier of finish() stands between this zero and the first addition
  __device__ __forceinline__ SrpMapBlock(const SrpCellArgs& k, int G, int blocks, int* clip_sum) {
    b = blockIdx.x / blocks;
    const int g0 = (blockIdx.x % blocks) * kSrpThreads + threadIdx.x;
    active = g0 < G;
    g = active ? g0 : G - 1;
    if (threadIdx.x == 0) *clip_sum = 0;
    centre = srp_frame_centre(k, b);
    wt = srp_frame_weights(k, b);
  }

  // power[B][G] takes the cell; the lanes' clipped terms add up in LDS and leave with one 64-bit integer atomic per workgroup
  __device__ __forceinline__ void finish(double* power, unsigned long long* clipped, int G, double acc, int clip, int* clip_sum) const {
    __syncthreads();                               // clip_sum is zero
    if (active) {
      power[size_t(b) * size_t(G) + g] = acc;
      if (clip) atomicAdd(clip_sum, clip);
    }
    __syncthreads();
    const int total = *clip_sum;
    if (threadIdx.x == 0 && total) atomicAdd(clipped + b, (unsigned long long)total);
  }
};

// ---- the level machinery of a zoom kernel: one workgroup per (frame, seed) runs every level ----
struct SrpZoomLds {
  double ctr[3];                                 // the level's centre
  double wave_p[kSrpThreads / 64];
  unsigned long long clip_sum;                   // 16^3 cells x P terms a level pass int32 from M = 1025 on
  int wave_g[kSrpThreads / 64];
  int stop;
};

// The record (thread 0's) begun from this workgroup's seed and the seed's position as the first centre.  -> the seed is absent
// (uniform): the record is then complete.  Its barrier also publishes what thread 0 wrote to LDS before the call.
__device__ __forceinline__ bool srp_zoom_begin(const pal_srp_peak* seeds, SrpZoomLds& s, pal_srp_zoom_record& rec) {
  rec.x = rec.y = rec.z = rec.power = 0.0;
  rec.clipped = 0;
  rec.seed = -1;
  rec.levels = 0;
  if (threadIdx.x == 0) {
    const pal_srp_peak seed = seeds[blockIdx.x];
    s.clip_sum = 0;
    s.stop = srp_zoom_absent(seed.index) ? 1 : 0;
    if (!s.stop) {
      rec.x = s.ctr[0] = seed.x;
      rec.y = s.ctr[1] = seed.y;
      rec.z = s.ctr[2] = seed.z;
      rec.seed = seed.index;
    }
  }
  __syncthreads();
  return s.stop != 0;
}

// The end of a level.  Every lane brings its best (my_p, my_g) by srp_before, my_g < 0 where it has none (NaN never enters), and its
// clipped terms (at most 16 cells x P < 2^31).  wave_arg63 reduces a wavefront, lane 63 of each writes LDS, and behind the first barrier
// thread 0 takes the best of the four - srp_before is a strict total order on distinct indices, so the lowest index among equal
// powers wins whatever the reduction's shape.  No cell: the zoom stops with a NaN power, the record keeping the centre this level
// started from.  Otherwise next(best_g, c3) gives the best cell's position - and writes the kernel's own next half-extent to LDS -
// and it becomes the record's and the next centre.  Behind the second barrier the next level, or stop, is in LDS and wave_p / wave_g
// are free again.  -> stop (uniform)
template <class NEXT>
__device__ __forceinline__ bool srp_zoom_pick(SrpZoomLds& s, double my_p, int my_g, int clip, int level, pal_srp_zoom_record& rec, NEXT next) {
  const int tid = threadIdx.x;
  wave_arg63(my_p, my_g, [](double pa, int ga, double pb, int gb) { return srp_before(pa, ga, pb, gb); });   // lane 63 holds the wave's best
  if ((tid & 63) == 63) {
    s.wave_p[tid >> 6] = my_p;
    s.wave_g[tid >> 6] = my_g;
  }
  if (clip) atomicAdd(&s.clip_sum, (unsigned long long)clip);
  __syncthreads();
  if (tid == 0) {
    double best_p = s.wave_p[0];
    int best_g = s.wave_g[0];
    for (int w = 1; w < kSrpThreads / 64; ++w)
      if (s.wave_g[w] >= 0 && (best_g < 0 || srp_before(s.wave_p[w], s.wave_g[w], best_p, best_g))) { best_p = s.wave_p[w]; best_g = s.wave_g[w]; }
    rec.clipped += int64_t(s.clip_sum);
    s.clip_sum = 0;
    if (srp_zoom_stops(best_g)) {
      s.stop = 1;
      rec.power = __builtin_nan("");
    } else {
      double c3[3];
      next(best_g, c3);
      rec.x = s.ctr[0] = c3[0];
      rec.y = s.ctr[1] = c3[1];
      rec.z = s.ctr[2] = c3[2];
      rec.power = best_p;
      rec.levels = level + 1;
    }
  }
  __syncthreads();
  return s.stop != 0;
}

}  // namespace pal
#endif
