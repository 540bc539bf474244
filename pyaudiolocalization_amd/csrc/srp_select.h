// srp_select.h - the body of k_srp_peaks and k_srp_doa_peaks (srp.hip): one frame's marks, then the K selection passes over the marked
// map.  The two kernels differ in how a cell is marked (`mark`: the box neighbourhood, or the direction grid's with azimuth wrapped)
// and in what a record's x, y, z hold (`pos`); the order of the peaks, the absent entries and the summary are one rule.
#pragma once
#include "engine.h"
#include "srp_math.h"

namespace pal {

constexpr int kSrpPeakThreads = 1024;

// what both peak kernels are told (srp.hip: launch_peaks fills it)
struct SrpPeakIo {
  const double* power;                  // [B][G]
  unsigned char* marks;                 // [B][G] (K > 0)
  pal_srp_peak* peaks;                  // [B][K] or nullptr
  pal_srp_frame* summary;               // [B] or nullptr
  const unsigned long long* clipped;    // [B] or nullptr (then 0)
  int G, K;
};

// One workgroup of kSrpPeakThreads, after the barrier behind its marks: pass k takes the block maximum - in the order power
// descending, index ascending - of the marked cells behind pass k - 1's pick, and thread 0 writes peaks[k] (absent: index -1, all else
// 0) and at last the summary.  power, marks: this frame's G cells; peaks: this frame's K records or nullptr; summary: this frame's or
// nullptr; clipped: this frame's counter or nullptr (then 0); best_p, best_g: kSrpPeakThreads entries of LDS each.
// pos(g, rec) fills rec.x, rec.y, rec.z of cell g.
template <class POS>
__device__ __forceinline__ void srp_select_peaks(const double* power, const unsigned char* marks, int G, int K, pal_srp_peak* peaks,
                                                 pal_srp_frame* summary, const unsigned long long* clipped, double* best_p, int* best_g,
                                                 POS pos) {
  const int tid = threadIdx.x;
  double prev_p = 0.0;
  int prev_g = -1, found = 0;
  for (int k = 0; k < K; ++k) {
    double my_p = 0.0;
    int my_g = -1;
    if (k == 0 || prev_g >= 0) {
      for (int g = tid; g < G; g += kSrpPeakThreads) {
        if (!marks[g]) continue;
        const double p = power[g];
        if (k > 0 && !srp_before(prev_p, prev_g, p, g)) continue;       // taken by an earlier pass
        if (my_g < 0 || srp_before(p, g, my_p, my_g)) { my_p = p; my_g = g; }
      }
    }
    best_p[tid] = my_p;
    best_g[tid] = my_g;
    __syncthreads();
    for (int half = kSrpPeakThreads / 2; half > 0; half >>= 1) {
      if (tid < half) {
        const int og = best_g[tid + half];
        const double op = best_p[tid + half];
        if (og >= 0 && (best_g[tid] < 0 || srp_before(op, og, best_p[tid], best_g[tid]))) { best_p[tid] = op; best_g[tid] = og; }
      }
      __syncthreads();
    }
    prev_p = best_p[0];
    prev_g = best_g[0];
    __syncthreads();                               // everyone has read the pick before the next pass overwrites it
    if (prev_g >= 0) ++found;
    if (tid == 0 && peaks) {
      pal_srp_peak rec;
      rec.x = rec.y = rec.z = rec.power = 0.0;
      rec.index = -1;
      rec.reserved = 0;
      if (prev_g >= 0) {
        pos(prev_g, rec);
        rec.power = prev_p;
        rec.index = prev_g;
      }
      peaks[k] = rec;
    }
  }
  if (tid == 0 && summary) {
    pal_srp_frame s;
    s.clipped = clipped ? int64_t(*clipped) : 0;
    s.n_peaks = found;
    s.reserved = 0;
    *summary = s;
  }
}

// A peak kernel's whole body, one workgroup per frame: mark(power, g) says whether cell g of this frame's map is a peak.
template <class MARK, class POS>
__device__ __forceinline__ void srp_peaks_frame(const SrpPeakIo& a, MARK mark, POS pos) {
  __shared__ double best_p[kSrpPeakThreads];
  __shared__ int best_g[kSrpPeakThreads];
  const int tid = threadIdx.x, b = blockIdx.x, G = a.G;
  const double* power = a.power + size_t(b) * size_t(G);
  unsigned char* marks = a.marks + size_t(b) * size_t(G);
  if (a.K > 0) {
    for (int g = tid; g < G; g += kSrpPeakThreads) marks[g] = mark(power, g) ? 1 : 0;
  }
  __syncthreads();
  srp_select_peaks(power, marks, G, a.K, a.peaks ? a.peaks + size_t(b) * size_t(a.K) : nullptr, a.summary ? a.summary + b : nullptr,
                   a.clipped ? a.clipped + b : nullptr, best_p, best_g, pos);
}

}  // namespace pal
