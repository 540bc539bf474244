// peaks.hip - peak selection and correlation metrics of the PHAT rows (gfx950).  Every route of the pair pipeline ends here:
//
//   three launches       k_peak_pivots + k_peak_stream + k_peak_finish<false> over stored rows
//   fused column pass    the column pass (pfa_cols_stats.h) brings the segments' results itself: k_peak_finish<true>
//   finishing passes     send every flagged row back through k_peak_finish
//
//   k_peak_pivots  one workgroup per row: an 8192-point block sample gives the shifts of the one-pass variances
//                  and two pivots that bracket the median of |corr| (6 sigma of the sample's rank error)
//   k_peak_stream  the row (n doubles, 0.7 MB at 44.1 kHz x 1 s) is cut into segments of a few 2048-element
//                  tiles; every 256-lane workgroup streams ONE segment with 16-byte loads, four in flight per
//                  lane plus a register double buffer: max / first argmax, min, shifted sums for the SNR and
//                  the 'adaptive' threshold, the highest local maximum, the count below the lower pivot, and
//                  the values between the pivots (compacted in LDS, flushed to the row's global list with one
//                  atomic per workgroup).  Small LDS, no inter-workgroup waits: bandwidth-bound, and light
//                  enough to run beside the FFT passes of the next launch group.
//   k_peak_finish  one workgroup per row (finish_row, a sequence of named steps): merges the segment results, repairs
//                  the best peak where the segments could not test it, SNR window, primary threshold - exact (a rank
//                  search inside the bracket list, radix select over the IEEE-754 bit pattern if the pivots missed or
//                  the list overflowed) or, fused column pass, an interval from the blocks' histograms that is made
//                  exact only when a comparison falls inside it - then scipy's find_peaks and the reference's
//                  fallback chain.
//
// Replaces utils.py:140-181 (threshold, scipy.signal.find_peaks(height, distance), the whole fallback chain,
// window filter, top-num_peaks), utils.py:228-250 (compute_snr / compute_peak_to_peak_ratio inputs) and
// np.max(corr) of main.py:223.
//
// The tiles of the stream are branch-free (guarded loads serialise on s_waitcnt); lane 0 / lane 63 of every
// wavefront leave their outer element's peak test to a short edge pass.
//
// scipy's find_peaks is evaluated lazily and exactly instead of materialising peak lists:
//   - a sample m is a peak iff it is the floor-midpoint of a plateau whose two outer neighbours
//     are strictly lower (end points never qualify)                      (_local_maxima_1d: is_peak, plateau_mid)
//   - the greedy distance suppression keeps peak X iff no KEPT peak of higher priority (height,
//     then position) lies closer than `distance`; that recursion is resolved depth first from the
//     candidate, with a memo, because chains of rising peaks are short   (_select_by_peak_distance: resolve)
//   - candidates are visited in descending priority inside the lag window until num_peaks are kept (select_peaks).
// Reductions: wavefront (64-lane) shuffles, then one LDS hop across the wavefronts.
//
// Order of the file, helpers before their users: workgroup primitives, rank search, local maxima, distance rule,
// selection, the three kernels, host entry points.  A helper that contains a barrier says so; it is called from
// workgroup-uniform control flow only.
#include <cfloat>
#include <climits>
#include <cmath>
#include <type_traits>

#include "engine.h"
#include "peak_types.h"
#include "reduce.h"

namespace pal {

namespace {

constexpr int kT = 512;           // lanes of the pivot and finish kernels (one row per workgroup)
constexpr int kNW = kT / 64;
constexpr int kTS = 256;          // lanes of the stream kernel (one segment per workgroup)
constexpr int kNWS = kTS / 64;
constexpr int kLoc = 3072;        // LDS capacity of one segment's share of it (a segment of 11 tiles brackets ~1100 values)
constexpr int kMaxTilesPerSeg = 11;
constexpr int kSample = 8192;     // block sample that places the pivots
constexpr int kBins = 2048;       // histogram bins (sample pivots, list search, radix digits)
constexpr int kSmall = 1024;      // exact rank search capacity
constexpr int kMemo = 1024;       // resolved peaks remembered per selection
constexpr int kStack = 64;        // depth of the suppression recursion
constexpr int kMaxStaged = 136;   // segments whose results the finish launch stages through LDS (the fused column pass has at most ceil(8192 / 62) = 133 blocks)
constexpr int kUnroll = 4;        // 16-byte loads in flight per lane
constexpr int kTile = kTS * kUnroll;   // element pairs per tile of the stream

// ------------------------------------------------------------------ workgroup primitives (pivot and finish kernels)
// Every one of them contains barriers.
struct Shared {
  unsigned hist[kBins];
  double small[kSmall];
  double red_d[kNW];
  double many[kNW * 8];
  int red_i[kNW];
  unsigned wave_tot[kNW];
  int count2;                            // fill of `small`
  int memo_pos[kMemo];
  int memo_kept[kMemo];
  int memo_n;
  int stack_pos[kStack];
  double stack_h[kStack];
  int stack_n;
  int flag;
  double bc_d[4];
  int bc_i[6];
  int sel_pos[PAL_MAX_PEAKS];            // selected peaks of the finish launch (written and read by lane 0)
  double sel_h[PAL_MAX_PEAKS];
};

__device__ double bsum(double v, Shared& s, int tid) { return block_sum<kNW>(v, s.red_d, tid); }
template <int N, int NW> __device__ void bsum_many(double (&v)[N], double* many, int tid) {   // N sums, one barrier pair
#pragma unroll
  for (int q = 0; q < N; ++q)
    for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_down(v[q], o, 64);
  __syncthreads();
  if ((tid & 63) == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) many[(tid >> 6) * N + q] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) {
    double r = 0;
    for (int k = 0; k < NW; ++k) r += many[k * N + q];
    v[q] = r;
  }
}
template <int MODE> __device__ void barg(double& v, int& i, Shared& s, int tid) {
  block_arg<MODE, kNW>(v, i, s.red_d, s.red_i, tid);
}

// exclusive prefix sum over the workgroup (one value per lane)
__device__ unsigned block_excl_scan(unsigned v, Shared& s, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  unsigned inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) s.wave_tot[wave] = inc;
  __syncthreads();
  unsigned before = 0;
  for (int k = 0; k < wave; ++k) before += s.wave_tot[k];
  return before + inc - v;
}

// wavefront-aggregated append to an LDS list (one LDS atomic per wavefront; no barrier, wavefront-uniform control flow)
__device__ __forceinline__ void append(bool pred, double v, double* list, int* counter, int cap, int lane) {
  const unsigned long long mask = __ballot(pred);
  if (mask == 0) return;
  const int leader = __ffsll((long long)mask) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(counter, __popcll(mask));
  base = __shfl(base, leader, 64);
  if (pred) {
    const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
    if (at < cap) list[at] = v;
  }
}

// ------------------------------------------------------------------ rank search
// An order statistic is found in two steps: a histogram (s.hist) places the rank in one bin, and the few values of that
// bin (s.small) are ranked exactly by counting.  The searches differ in their first pass only: linear bins over a row's
// bracket list (list_select), a known interval of the row (interval_select), radix digits of the row (radix_select).
// The three are kept out of line: each has two call sites in the finish kernel, and inlined there they cost it registers
// and scratch (list_select alone holds sixteen list values per lane between its passes).

// zeroes s.hist (no barrier: the caller's next one publishes it)
__device__ __forceinline__ void clear_hist(Shared& s, int tid) {
  for (int k = tid; k < kBins; k += kT) s.hist[k] = 0;
}

struct RankBin { unsigned bin, inner, pop; };   // bin of s.hist that holds a rank, the rank inside that bin, the bin's population

// bins of s.hist that hold the N (one or two) 0-based ranks `rank`: one scan, 2 bins per lane (contains barriers).
// A rank beyond the histogram's total reports the last bin with population 0.
template <int N> __device__ void find_bins(Shared& s, int tid, const unsigned (&rank)[N], RankBin (&out)[N]) {
  static_assert(N == 1 || N == 2, "three broadcast words per rank in s.bc_i");
  constexpr int kPer = kBins / kT;                  // consecutive bins owned by one lane
  unsigned h[kPer], own = 0;
#pragma unroll
  for (int q = 0; q < kPer; ++q) { h[q] = s.hist[kPer * tid + q]; own += h[q]; }
  unsigned ex = block_excl_scan(own, s, tid);
  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) s.bc_i[3 * j] = -1;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (rank[j] >= ex && rank[j] < ex + h[q]) { s.bc_i[3 * j] = kPer * tid + q; s.bc_i[3 * j + 1] = int(rank[j] - ex); s.bc_i[3 * j + 2] = int(h[q]); }
    ex += h[q];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if (s.bc_i[3 * j] < 0) out[j] = RankBin{unsigned(kBins - 1), 0u, 0u};
    else out[j] = RankBin{unsigned(s.bc_i[3 * j]), unsigned(s.bc_i[3 * j + 1]), unsigned(s.bc_i[3 * j + 2])};
  }
  __syncthreads();
}

// the one-rank use (contains barriers)
__device__ void find_bin(Shared& s, int tid, unsigned rank, unsigned& bin, unsigned& inner, unsigned& pop) {
  const unsigned r[1] = {rank};
  RankBin at[1];
  find_bins<1>(s, tid, r, at);
  bin = at[0].bin; inner = at[0].inner; pop = at[0].pop;
}

// exact value of 0-based rank `inner` among the s.count2 values collected in s.small (false: more than its capacity);
// contains barriers
__device__ bool small_rank(Shared& s, int tid, unsigned inner, double& out) {
  if (s.count2 > kSmall) { __syncthreads(); return false; }
  const int m = s.count2;
  for (int e = tid; e < m; e += kT) {
    const double v = s.small[e];
    unsigned below = 0;
    for (int j = 0; j < m; ++j) {
      const double u = s.small[j];
      below += (u < v) || (u == v && j < e);
    }
    if (below == inner) s.bc_d[0] = v;
  }
  __syncthreads();
  out = s.bc_d[0];
  __syncthreads();
  return true;
}

// survivors of a search over the stored row: |c[i]| of every sample with keep(|c[i]|) goes to s.small, their number to
// s.count2 (which may exceed the capacity kSmall); four loads in flight per lane; contains barriers
template <class Keep> __device__ __forceinline__ void collect_row(Shared& s, int tid, const double* __restrict__ c, int n, Keep keep) {
  if (tid == 0) s.count2 = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += 4 * kT) {
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * kT + tid;
      v[u] = i < n ? fabs(c[i]) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) append(i0 + u * kT + tid < n && keep(v[u]), v[u], s.small, &s.count2, kSmall, tid & 63);
  }
  __syncthreads();
}

// ---- exact rank inside the row's bracket list (global memory, L2-resident) whose values lie in [lo, hi] ----
// linear bins spread the bracket over the histogram; the winning bin (a handful of values) is ranked by counting.
// returns false when that bin is too crowded for the exact search (caller falls back to the radix select); contains barriers
__device__ __noinline__ bool list_select(Shared& s, int tid, const double* __restrict__ list, int cnt, unsigned rank, double lo, double hi,
                            double& out) {
  constexpr int kKeep = 16;                                    // list values a lane keeps in registers between the two passes
  clear_hist(s, tid);
  if (tid == 0) s.count2 = 0;
  __syncthreads();
  const double span = hi - lo;
  const double inv = (span > 0 && isfinite(span)) ? double(kBins - 1) / span : 0.0;
  auto bin_of = [&](double v) {
    int b = int((v - lo) * inv);
    return b < 0 ? 0 : (b > kBins - 1 ? kBins - 1 : b);
  };
  double keep[kKeep];
#pragma unroll
  for (int q = 0; q < kKeep; ++q) {                            // all loads in flight together
    const int e = tid + q * kT;
    keep[q] = e < cnt ? list[e] : 0.0;
  }
#pragma unroll
  for (int q = 0; q < kKeep; ++q)
    if (tid + q * kT < cnt) atomicAdd(&s.hist[bin_of(keep[q])], 1u);
  for (int e = tid + kKeep * kT; e < cnt; e += kT) atomicAdd(&s.hist[bin_of(list[e])], 1u);
  __syncthreads();
  unsigned bin, inner, pop;
  find_bin(s, tid, rank, bin, inner, pop);
  if (pop == 0 || pop > unsigned(kSmall)) return false;
  // the winning bin holds a handful of values: a lane that owns one takes a slot with its own LDS atomic
  auto take = [&](double v) {
    if (unsigned(bin_of(v)) != bin) return;
    const int at = atomicAdd(&s.count2, 1);
    if (at < kSmall) s.small[at] = v;
  };
#pragma unroll
  for (int q = 0; q < kKeep; ++q)
    if (tid + q * kT < cnt) take(keep[q]);
  for (int e = tid + kKeep * kT; e < cnt; e += kT) take(list[e]);
  __syncthreads();
  return small_rank(s, tid, inner, out);
}

// Exact order statistic `rank_in` (0-based, counted inside the interval) of |c| among the row's samples with
// lo <= |c| < hi: one pass over the stored row.  The fused column pass knows the interval from its histograms (about
// 0.2 % of the row); used only when a threshold comparison falls inside mult x that interval.  Contains barriers.
__device__ __noinline__ bool interval_select(Shared& s, int tid, const double* __restrict__ c, int n, double lo, double hi, unsigned rank_in,
                                double& out) {
  collect_row(s, tid, c, n, [&](double v) { return v >= lo && v < hi; });
  if (unsigned(s.count2) <= rank_in) { __syncthreads(); return false; }
  return small_rank(s, tid, rank_in, out);
}

// ---- fallback: radix select over the 63 magnitude bits, re-reading the row (contains barriers) ----
__device__ __forceinline__ int digit_shift(int level) { return level < 5 ? 52 - 11 * level : 0; }
__device__ __forceinline__ unsigned digit_mask(int level) { return level < 5 ? 0x7FFu : 0xFFu; }
__device__ __forceinline__ unsigned long long mag_key(double x) { return (unsigned long long)__double_as_longlong(fabs(x)); }

__device__ __noinline__ double radix_select(const double* c, int n, int tid, Shared& s, unsigned rank) {
  unsigned long long prefix = 0;
  unsigned inner = rank, bin, pop;
  for (int level = 0; level < 6; ++level) {
    clear_hist(s, tid);
    __syncthreads();
    const int sh = digit_shift(level);
    const unsigned mk_ = digit_mask(level);
    for (int i = tid; i < n; i += kT) {
      const unsigned long long key = mag_key(c[i]);
      if (level == 0 || (key >> digit_shift(level - 1)) == prefix) atomicAdd(&s.hist[unsigned(key >> sh) & mk_], 1u);
    }
    __syncthreads();
    find_bin(s, tid, inner, bin, inner, pop);
    prefix = (prefix << (level < 5 ? 11 : 8)) | bin;
    if (pop <= unsigned(kSmall) && level < 5) {                // few survivors: rank them exactly
      collect_row(s, tid, c, n, [&](double v) { return (mag_key(v) >> sh) == prefix; });
      double r = 0;
      small_rank(s, tid, inner, r);
      return r;
    }
  }
  return __longlong_as_double((long long)prefix);   // every magnitude bit fixed: all survivors are equal
}

// ------------------------------------------------------------------ local maxima (scipy _local_maxima_1d)
// Is sample m a peak, given xl = c[m - 1], x = c[m], xr = c[m + 1] already loaded (1 <= m <= n - 2)?  A strict peak, or
// the floor-midpoint of a plateau whose two outer neighbours are strictly lower; a plateau that touches an end of the
// row is none.  The peak's height is x.  Memory is read on a tie only, so callers batch the three independent loads of
// many samples in front of this test.
__device__ __forceinline__ bool is_peak(const double* c, int n, int m, double xl, double x, double xr) {
  if (xl < x && xr < x) return true;
  if (!(xl == x || xr == x)) return false;
  int l = m, r = m;                                            // a plateau: walk to both edges
  while (l > 0 && c[l - 1] == x) --l;
  while (r < n - 1 && c[r + 1] == x) ++r;
  if (l < 1 || r > n - 2) return false;
  return c[l - 1] < x && c[r + 1] < x && m == (l + r) / 2;
}

// The plateau of height x that STARTS at m (c[m - 1] < x == c[m + 1], 1 <= m <= n - 2): walks to its right edge once and
// gives its floor-midpoint if the far neighbour is lower; false if not (or if the plateau runs into the row's end).
// For passes that meet every sample of a plateau and must count it once: the stream's tiles, the row tests of finish_row.
__device__ __forceinline__ bool plateau_mid(const double* c, int n, int m, double x, int& mid) {
  int q = m + 1;
  while (q < n - 1 && c[q] == x) ++q;
  if (!(c[q] < x)) return false;
  mid = (m + q - 1) / 2;
  return true;
}

// ------------------------------------------------------------------ distance rule (scipy _select_by_peak_distance)
// ---- greedy distance suppression, resolved from one candidate ----
__device__ int memo_find(const Shared& s, int pos) {
  for (int k = 0; k < s.memo_n; ++k)
    if (s.memo_pos[k] == pos) return s.memo_kept[k];
  return -1;
}

// returns 1 kept, 0 suppressed, -1 overflow; contains barriers, workgroup-uniform control flow
__device__ __forceinline__ int resolve(const double* c, int n, int dist, int tid, Shared& s, int pos0, double h0, int memo_cap, int stack_cap) {
  if (tid == 0) { s.stack_n = 1; s.stack_pos[0] = pos0; s.stack_h[0] = h0; s.flag = 0; }
  __syncthreads();
  for (int guard = 0; guard < 100000; ++guard) {
    const int depth = s.stack_n;
    if (depth == 0) break;
    const int p = s.stack_pos[depth - 1];
    const double h = s.stack_h[depth - 1];
    __syncthreads();
    if (memo_find(s, p) >= 0) {                       // resolved while deeper frames ran
      if (tid == 0) s.stack_n = depth - 1;
      __syncthreads();
      continue;
    }
    int any_kept = 0;                                 // neighbours closer than dist with higher priority
    double bh = 0;
    int bm = -1;
    for (int o = tid - (dist - 1); o <= dist - 1; o += kT) {
      if (o == 0) continue;
      const int m = p + o;
      if (m < 1 || m > n - 2) continue;
      const double xl = c[m - 1], xr = c[m + 1];             // the three reads are independent: one round trip, not three
      const double hm = c[m];
      if (!is_peak(c, n, m, xl, hm, xr)) continue;
      if (higher(hm, m, h, p)) {
        const int st = memo_find(s, m);
        if (st == 1) any_kept = 1;
        else if (st < 0 && (bm < 0 || higher(hm, m, bh, bm))) { bh = hm; bm = m; }
      }
    }
    any_kept = __syncthreads_or(any_kept);
    barg<2>(bh, bm, s, tid);
    if (tid == 0) {
      if (any_kept || bm < 0) {
        if (s.memo_n < memo_cap) {
          s.memo_pos[s.memo_n] = p;
          s.memo_kept[s.memo_n] = any_kept ? 0 : 1;
          ++s.memo_n;
        } else {
          s.flag = 1;
        }
        s.stack_n = depth - 1;
      } else if (depth < stack_cap) {
        s.stack_pos[depth] = bm;
        s.stack_h[depth] = bh;
        s.stack_n = depth + 1;
      } else {
        s.flag = 1;
      }
    }
    __syncthreads();
    if (s.flag) return -1;
  }
  __syncthreads();
  const int st = memo_find(s, pos0);
  __syncthreads();
  return st < 0 ? -1 : st;
}

// ---- the same decision without capacity limits: scipy's greedy pass itself, over every peak above the candidate ----
// resolve() answers "is the candidate kept?" depth first with an on-chip memo (1024 resolved peaks, 64 frames): enough for any
// PHAT row met so far, but utils.py:152 has no such limit.  When it overflows, the row takes this path: a bitmap of the row's
// peaks (scipy's _local_maxima_1d, plateau midpoints included) and a bitmap of the positions already suppressed, both in
// global memory; then _select_by_peak_distance literally - the highest peak not yet suppressed is kept and suppresses every
// position closer than `distance` - until the candidate's priority is reached.  Milliseconds per row, exact for any input.
__device__ int resolve_slow(const double* c, int n, int dist, int tid, Shared& s, unsigned* bits, int pos0, double h0) {
  const int words = (n + 31) / 32;
  unsigned* peak = bits;                                       // bit m: sample m is a peak
  unsigned* gone = bits + words;                               // bit m: suppressed (or kept: not to be found again)
  for (int w = tid; w < words; w += kT) {
    unsigned pk = 0;
    for (int b = 0; b < 32; ++b) {
      const int m = 32 * w + b;
      if (m < 1 || m > n - 2) continue;
      if (is_peak(c, n, m, c[m - 1], c[m], c[m + 1])) pk |= 1u << b;
    }
    peak[w] = pk;
    gone[w] = 0;
  }
  __syncthreads();
  for (int guard = 0; guard < n; ++guard) {
    // the highest peak above the candidate that is still standing
    double bh = 0;
    int bm = -1;
    for (int w = tid; w < words; w += kT) {
      unsigned live = peak[w] & ~gone[w];
      while (live) {
        const int b = __ffs(int(live)) - 1;
        live &= live - 1;
        const int m = 32 * w + b;
        const double hm = c[m];
        if (higher(hm, m, h0, pos0) && (bm < 0 || higher(hm, m, bh, bm))) { bh = hm; bm = m; }
      }
    }
    barg<2>(bh, bm, s, tid);
    if (bm < 0) break;                                         // nothing above the candidate is left: it is kept
    if (bm - pos0 < dist && pos0 - bm < dist) return 0;        // a kept higher peak closer than `distance`
    const int lo = bm - (dist - 1) > 0 ? bm - (dist - 1) : 0, hi = bm + (dist - 1) < n - 1 ? bm + (dist - 1) : n - 1;
    for (int m = lo + tid; m <= hi; m += kT) atomicOr(&gone[m >> 5], 1u << (m & 31));
    __syncthreads();
  }
  return 1;
}

// ------------------------------------------------------------------ selection (utils.py:152-179: height, distance, window, top num_peaks)
__device__ __forceinline__ bool in_window(int m, int n2, double fs, double med) {
  return fabs(double(m - (n2 - 1)) / fs) <= med;       // abs(time_lags[k]) <= max_expected_delay (utils.py:163)
}

// highest-priority peak with height >= thr inside [wlo, whi] (exact window test when windowed) and
// priority below (bound_h, bound_m); returns false when none
struct SelArgs {            // by value: a reference to the kernel's argument struct would force it (and the address
  int n, n2, dist, num_peaks;   // space of every pointer in it) through private memory
  double fs, med;
  unsigned* bits;           // this row's bitmaps for resolve_slow
  int memo_cap, stack_cap;
};

__device__ __forceinline__ bool next_candidate(const SelArgs a, const double* c, int tid, Shared& s, double thr, bool windowed, int wlo,
                               int whi, double bound_h, int bound_m, double& ch, int& cm) {
  double bh = 0;
  int bm = -1;
  // four samples per lane and round with all twelve loads in flight (the scan is latency-bound: a dependent
  // round trip per sample made it the longest phase of the finish kernel); plateaus take the exact slow test
  for (int m0 = wlo + tid; m0 <= whi; m0 += 4 * kT) {
    double xl[4], xc[4], xr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = m0 + u * kT;
      const int mm = m <= whi ? m : whi;                       // wlo >= 1 and whi <= n - 2: all three reads are in range
      xl[u] = c[mm - 1];
      xc[u] = c[mm];
      xr[u] = c[mm + 1];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = m0 + u * kT;
      if (m > whi) continue;
      const double hm = xc[u];
      if (!is_peak(c, a.n, m, xl[u], hm, xr[u])) continue;
      if (!(hm >= thr)) continue;
      if (windowed && !in_window(m, a.n2, a.fs, a.med)) continue;
      if (!higher(bound_h, bound_m, hm, m)) continue;
      if (bm < 0 || higher(hm, m, bh, bm)) { bh = hm; bm = m; }
    }
  }
  barg<2>(bh, bm, s, tid);
  ch = bh;
  cm = bm;
  return bm >= 0;
}

// top-num_peaks kept peaks >= thr in the window; returns count or -1 on overflow.  The threshold may be known as an
// interval only (tlo <= thr <= thi, fused column pass): candidates arrive in descending height, one at or above thi
// passes, one below tlo ends the search, and for one in between the function returns -2: the caller makes the
// threshold exact (tlo == thi) and calls again.
__device__ __forceinline__ int select_peaks(const SelArgs a, const double* c, int tid, Shared& s, double tlo, double thi,
                            bool windowed, int wlo, int whi, double first_h, int first_m) {
  if (tid == 0) s.memo_n = 0;
  __syncthreads();
  double bound_h = INFINITY;
  int bound_m = INT_MAX;
  int count = 0;
  bool use_first = first_m >= 0;
  while (count < a.num_peaks) {
    double ch;
    int cm;
    if (use_first) {
      ch = first_h; cm = first_m; use_first = false;
    } else {
      if (!next_candidate(a, c, tid, s, tlo, windowed, wlo, whi, bound_h, bound_m, ch, cm)) break;
      if (!(ch >= thi)) return -2;                             // inside the threshold's interval (never when tlo == thi)
    }
    int st = resolve(c, a.n, a.dist, tid, s, cm, ch, a.memo_cap, a.stack_cap);
    if (st < 0 && a.bits) {                                              // memo or stack exhausted: the exact slow path, then a fresh memo
      st = resolve_slow(c, a.n, a.dist, tid, s, a.bits, cm, ch);
      __syncthreads();
      if (tid == 0) s.memo_n = 0;
      __syncthreads();
    }
    if (st < 0) return -1;
    if (st == 1) {                                             // (the list lives in LDS: 48 registers per lane otherwise)
      if (tid == 0) { s.sel_pos[count] = cm; s.sel_h[count] = ch; }
      ++count;
    }
    bound_h = ch;
    bound_m = cm;
  }
  return count;
}

// ------------------------------------------------------------------ kernel 1: pivots
// A block sample of the row (16 coalesced runs of 512 values spread over it) gives the shifts of the one-pass variances
// and the pivots that bracket the median.
__global__ __launch_bounds__(kT) void k_peak_pivots(PeakArgs a) {
  __shared__ Shared s;
  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  const double* c = a.corr + size_t(row) * a.stride;
  const int n = a.n;
  constexpr int kRuns = kSample / kT;                          // values per lane; `ns` of them are real in the whole workgroup
  const int ns = n < kSample ? n : kSample;
  double sv[kRuns];
  bool real[kRuns];
#pragma unroll
  for (int q = 0; q < kRuns; ++q) {
    const int si = tid + q * kT;
    const size_t at = n <= kSample ? size_t(si) : size_t((long long)q * (n - kT) / (kRuns - 1)) + tid;
    real[q] = si < ns;
    sv[q] = real[q] ? c[at] : 0.0;
  }
  // Lower bounds for the stream launch: the sample's maximum, and its highest strict peak (inside a run the lanes
  // tid -/+ 1 of the same wavefront hold the neighbours).  A sample below them can be neither the row's maximum nor its
  // highest local maximum, which lets the stream keep the index bookkeeping and the neighbour tests out of its loop.
  const int lane = tid & 63;
  double vm = -INFINITY, pm = -INFINITY;
#pragma unroll
  for (int q = 0; q < kRuns; ++q) {
    const double x = sv[q];
    const double left = from_lower_lane(x), right = from_upper_lane(x);
    vm = real[q] ? fmax(vm, x) : vm;
    const bool inner = real[q] && lane >= 1 && lane <= 62 && tid + 1 + q * kT < ns;
    pm = inner && left < x && right < x ? fmax(pm, x) : pm;
  }
  vm = block_max<kNW>(vm, s.red_d, tid);
  __syncthreads();
  pm = block_max<kNW>(pm, s.red_d, tid);
  __syncthreads();
  double ssum = 0, sabs = 0;
#pragma unroll
  for (int q = 0; q < kRuns; ++q) {
    ssum += sv[q];                                             // (values that are not real are zero)
    sabs += fabs(sv[q]);
  }
  double both[2] = {ssum, sabs};
  bsum_many<2, kNW>(both, s.many, tid);
  const double k0 = both[0] / double(ns);                     // ~ mean(x)
  const double ka = both[1] / double(ns);                     // ~ mean(|x|)
  double lo = 0, hi = INFINITY;
  if (a.method == 0) {
    const unsigned r1 = unsigned((n - 1) / 2), r2 = unsigned(n / 2);   // ranks of the median's one or two order statistics
    clear_hist(s, tid);
    __syncthreads();
    const double top = ka > 0 ? 4.0 * ka : 1.0;               // median <= 2 mean for non-negative data
    const double inv = double(kBins - 1) / top;
#pragma unroll
    for (int q = 0; q < kRuns; ++q) {
      if (real[q]) {
        int b = int(fabs(sv[q]) * inv);
        atomicAdd(&s.hist[b < kBins - 1 ? b : kBins - 1], 1u);
      }
    }
    __syncthreads();
    // 6 sigma of an independent sample median's rank.  The block sample is not independent (neighbouring lags of a
    // PHAT sequence are correlated): at 4 sigma 10 of 40320 metric rows missed and paid the radix select, whose
    // row alone then takes longer than the whole launch.
    const int margin = int(3.0 * sqrt(double(ns))) + 8;
    const long long c1 = (long long)r1 * ns / n, c2 = (long long)r2 * ns / n;
    const unsigned slo = unsigned(c1 - margin > 0 ? c1 - margin : 0);
    const unsigned shi = unsigned(c2 + margin < ns - 1 ? c2 + margin : ns - 1);
    const unsigned ranks[2] = {slo, shi};
    RankBin at[2];
    find_bins<2>(s, tid, ranks, at);                           // (one scan, half the barriers of two searches)
    lo = double(at[0].bin) / inv;
    hi = at[1].bin >= unsigned(kBins - 1) ? INFINITY : double(at[1].bin + 1) / inv;
    if (slo == 0) lo = 0;
    if (shi == unsigned(ns - 1)) hi = INFINITY;
  }
  if (tid == 0) {
    RowPre pre;
    pre.k0 = k0; pre.ka = ka; pre.lo = lo; pre.hi = hi;
    pre.vfloor = vm; pre.pfloor = pm;
    a.pre[row] = pre;
    a.gcount[row] = 0;      // the row's bracket list starts empty (the launch behind this one fills it)
  }
}

// ------------------------------------------------------------------ kernel 2: stream
struct StreamWave {                      // one wavefront's share of a segment's statistics
  double vmax, vmin, hb, sums[5];
  int imax, mb;
};

struct StreamShared {
  double list[kLoc + 1];                 // + one dump slot for the unconditional stores of values outside the bracket
  StreamWave wave[kNWS];
  int count;
  int bc_i;
};

struct Stream {            // per-lane accumulators of the single pass over a segment
  double vmax, vmin, hb;
  int imax, mb;            // < 0: nothing recorded yet
  double s1, s2, a1, a2;   // sums of (x-K0), (x-K0)^2, (|x|-Ka), (|x|-Ka)^2
  int below;
};

// statistics of one sample: selects instead of branches (the loop is issue-bound, and a divergent branch costs
// more scalar bookkeeping than the handful of conditional moves it would skip).  First occurrence wins inside a
// lane because the lane meets its samples in increasing index order.  vmax / vmin / hb start at -inf / +inf / -inf.
template <bool FULL> __device__ __forceinline__ void visit_max(Stream& t, double x, int i, bool valid) {
  const bool up = (FULL || valid) && x > t.vmax;
  t.imax = up ? i : t.imax;
  t.vmax = up ? x : t.vmax;
}
template <bool FULL> __device__ __forceinline__ void visit(Stream& t, double x, bool valid, double k0, double ka) {
  t.vmin = (FULL || valid) ? fmin(t.vmin, x) : t.vmin;
  const double d = (FULL || valid) ? x - k0 : 0.0, e = (FULL || valid) ? fabs(x) - ka : 0.0;
  t.s1 += d;
  t.s2 = __builtin_fma(d, d, t.s2);
  t.a1 += e;
  t.a2 = __builtin_fma(e, e, t.a2);
}

// x at index i with neighbours l (i-1) and r (i+1): the highest local maximum so far (scipy's floor-midpoint of a
// plateau; inside a lane a later peak of equal height wins, as in the priority order).  `ok` carries the lane
// mask (the outer element of lane 0 / 63 belongs to the edge pass) and, outside full tiles, the range 1 <= i <= n-2.
// Returns true when the sample starts a plateau (r == x), which the caller resolves from memory in a rarely
// taken branch.
__device__ __forceinline__ bool peak_fast(Stream& t, int i, bool ok, double l, double x, double r) {
  const bool cand = ok && l < x && x >= t.hb;
  const bool pk = cand && r < x;
  t.hb = pk ? x : t.hb;
  t.mb = pk ? i : t.mb;
  return cand && r == x;
}

// plateau that starts at absolute index i: find its right edge in memory; indices are recorded relative to `lane_off`
__device__ __forceinline__ void peak_plateau(Stream& t, const double* c, int n, int i, double x, int lane_off) {
  int m;
  if (!plateau_mid(c, n, i, x, m)) return;
  m -= lane_off;
  if (t.mb < 0 || higher(x, m, t.hb, t.mb)) { t.hb = x; t.mb = m; }
}

// edge-pass form: neighbours read from memory
__device__ __forceinline__ void peak_test(Stream& t, const double* c, int n, int i, double l, double x, double r, int lane_off) {
  if (peak_fast(t, i - lane_off, i >= 1 && i <= n - 2, l, x, r)) peak_plateau(t, c, n, i, x, lane_off);
}

__global__ __launch_bounds__(kTS) void k_peak_stream(PeakArgs a) {
  __shared__ StreamShared s;
  const int tid = threadIdx.x, lane = tid & 63;
  const int S = a.splits;
  const int row = blockIdx.x / S, seg = blockIdx.x % S;
  const double* c = a.corr + size_t(row) * a.stride;
  const int n = a.n;
  const bool want_median = a.method == 0;
  const RowPre pre = load_pre(a.pre, row);
  const double k0 = pre.k0, ka = pre.ka, lo = pre.lo, hi = pre.hi;
  const double floor = fmin(pre.vfloor, pre.pfloor);           // (-inf when the sample held no strict peak: every tile is examined)
  if (tid == 0) s.count = 0;
  __syncthreads();

  // ---- branch-free tiles of kUnroll 16-byte loads per lane, then a short guarded tail ----
  Stream t;
  t.vmax = t.hb = -INFINITY;
  t.vmin = INFINITY;
  t.imax = t.mb = -1;
  t.s1 = t.s2 = t.a1 = t.a2 = 0;
  t.below = 0;
  const bool aligned = (reinterpret_cast<size_t>(c) & 15) == 0;
  const int npair = (n + 1) / 2;
  // this workgroup's share: a whole number of tiles, so segment borders fall on multiples of 128 elements
  const int per_seg = a.tiles_per_seg * kTile;
  const int p_lo = seg * per_seg < npair ? seg * per_seg : npair;
  const int p_hi = p_lo + per_seg < npair ? p_lo + per_seg : npair;
  const int both = p_hi < (n - 1) / 2 ? p_hi : (n - 1) / 2;    // pairs below `both`: both elements valid and at most n - 2
  const int full = p_lo + (both > p_lo ? (both - p_lo) / kTile * kTile : 0);   // end of the branch-free tiles
  // Element e = 2p (+1) of pair p; lane = p % 64.  Neighbours come from the adjacent lanes; the first element
  // of lane 0 and the second of lane 63 (e % 128 == 0 / 127) are peak-tested by the edge pass below instead.
  // One tile = kUnroll element pairs per lane.  Statistics and peak tests per element; the bracket values of the
  // whole tile are appended with ONE LDS atomic per wavefront: per element a ballot gives the lane's rank
  // (mbcnt) and the wavefront's count (scalar popcount), the running scalar total is the tile's reservation.
  const bool not0 = lane != 0, not63 = lane != 63;
  // the edge elements e = 128 q and e = 128 q + 127 of this segment (at most two per lane): their values are requested
  // now and looked at behind the stream; the neighbours are only read for the few that reach the bounds
  static_assert(kMaxTilesPerSeg * kTile * 2 / 64 <= 2 * kTS, "two edge elements per lane");
  int edge_at[2];
  double edge_x[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int j = tid + r * kTS;
    const int e = 2 * p_lo + (j >> 1) * 128 + ((j & 1) ? 127 : 0);
    const bool ok = 2 * p_lo + 64 * j < 2 * p_hi && e >= 1 && e <= n - 2 && e < 2 * p_hi;
    edge_at[r] = ok ? e : -1;
    edge_x[r] = ok ? c[e] : -INFINITY;
  }
  auto consume_tile = [&](const double* xa, const double* xb, int pair0u, auto full_tag) {
    constexpr bool FULL = decltype(full_tag)::value;           // full tiles: every element valid, none at index 0 or n - 1
    const int pair0 = pair0u + tid;                            // pair0u: the tile's first pair (wave-uniform)
    int off[2 * kUnroll];
    int run = 0;
    unsigned long long reach = 0;                              // lanes with a sample at or above the pivot launch's bounds
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const int e0 = 2 * (pair0 + k * kTS);
      const bool va = FULL || e0 < n, vb = FULL || e0 + 1 < n;
      visit<FULL>(t, xa[k], va, k0, ka);
      visit<FULL>(t, xb[k], vb, k0, ka);
      reach |= __ballot((va && xa[k] >= floor) || (vb && xb[k] >= floor));
      if (want_median) {
        const double ma = fabs(xa[k]), mb_ = fabs(xb[k]);
        t.below += int(va && ma < lo) + int(vb && mb_ < lo);
        const bool ha = va && ma >= lo && ma <= hi, hb_ = vb && mb_ >= lo && mb_ <= hi;
        const unsigned long long m0 = __ballot(ha), m1 = __ballot(hb_);
        // slot inside the tile's reservation, or the dump slot kLoc for values outside the bracket: the LDS store
        // below is unconditional (a guarded store costs a divergent branch per sample)
        const int ra = run + int(__builtin_amdgcn_mbcnt_hi(unsigned(m0 >> 32), __builtin_amdgcn_mbcnt_lo(unsigned(m0), 0u)));
        run += __popcll(m0);
        const int rb = run + int(__builtin_amdgcn_mbcnt_hi(unsigned(m1 >> 32), __builtin_amdgcn_mbcnt_lo(unsigned(m1), 0u)));
        run += __popcll(m1);
        off[2 * k] = ha ? ra : kLoc;
        off[2 * k + 1] = hb_ ? rb : kLoc;
      }
    }
    if (reach) {
      // about one tile in ten holds a sample that can be the row's maximum or its highest local maximum (none below
      // the bounds can): only there the index bookkeeping and the neighbour tests run
      bool plateau = false;
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) {
        const int e0 = 2 * (pair0 + k * kTS);
        // indices are recorded relative to the lane's own offset 2 tid: the recorded value is wave-uniform (a scalar
        // operand of the select instead of a vector add per sample); the lane offset is added back after the loop
        const int u0 = 2 * (pair0u + k * kTS);
        const bool va = FULL || e0 < n, vb = FULL || e0 + 1 < n;
        const double left = from_lower_lane(xb[k]);
        const double right = from_upper_lane(xa[k]);
        visit_max<FULL>(t, xa[k], u0, va);
        visit_max<FULL>(t, xb[k], u0 + 1, vb);
        plateau |= peak_fast(t, u0, FULL ? not0 : (not0 && va && e0 >= 1 && e0 <= n - 2), left, xa[k], xb[k]);
        plateau |= peak_fast(t, u0 + 1, FULL ? not63 : (not63 && vb && e0 + 1 <= n - 2), xa[k], xb[k], right);
      }
      if (__ballot(plateau)) {                                 // equal neighbours somewhere in the tile: the exact, slow test
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
          const int e0 = 2 * (pair0 + k * kTS);
          const bool va = FULL || e0 < n, vb = FULL || e0 + 1 < n;
          const double left = from_lower_lane(xb[k]);
          if (va && lane != 0 && e0 >= 1 && e0 <= n - 2 && left < xa[k] && xb[k] == xa[k]) peak_plateau(t, c, n, e0, xa[k], 2 * tid);
          const double right = from_upper_lane(xa[k]);
          if (vb && lane != 63 && e0 + 1 <= n - 2 && xa[k] < xb[k] && right == xb[k]) peak_plateau(t, c, n, e0 + 1, xb[k], 2 * tid);
        }
      }
    }
    if (want_median && run > 0) {                              // wavefront-uniform
      int base = 0;
      if (lane == 0) base = atomicAdd(&s.count, run);
      base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) {
        const int ia = off[2 * k] < kLoc ? min(base + off[2 * k], kLoc) : kLoc;
        const int ib = off[2 * k + 1] < kLoc ? min(base + off[2 * k + 1], kLoc) : kLoc;
        s.list[ia] = fabs(xa[k]);
        s.list[ib] = fabs(xb[k]);
      }
    }
  };
  // register double buffer: the next tile's loads are in flight while this one is consumed
  if (aligned) {
    double2 cur[kUnroll], nxt[kUnroll];
    if (p_lo < full) {
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) cur[k] = *reinterpret_cast<const double2*>(c + 2 * (p_lo + k * kTS + tid));
    }
    for (int base = p_lo; base < full; base += kTile) {
      const int ahead = base + kTile < full ? base + kTile : base;    // last round re-reads its own tile: no branch
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) nxt[k] = *reinterpret_cast<const double2*>(c + 2 * (ahead + k * kTS + tid));
      double xa[kUnroll], xb[kUnroll];
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) { xa[k] = cur[k].x; xb[k] = cur[k].y; }
      consume_tile(xa, xb, base, std::true_type{});
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) cur[k] = nxt[k];
    }
  } else {
    for (int base = p_lo; base < full; base += kTile) {
      double xa[kUnroll], xb[kUnroll];
#pragma unroll
      for (int k = 0; k < kUnroll; ++k) {
        xa[k] = c[2 * (base + k * kTS + tid)];
        xb[k] = c[2 * (base + k * kTS + tid) + 1];
      }
      consume_tile(xa, xb, base, std::true_type{});
    }
  }
  if (full < p_hi) {                                           // tail: one guarded tile
    double xa[kUnroll], xb[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const int e0 = 2 * (full + k * kTS + tid);
      xa[k] = e0 < n ? c[e0] : 0.0;
      xb[k] = e0 + 1 < n ? c[e0 + 1] : 0.0;
    }
    consume_tile(xa, xb, full, std::false_type{});
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {                                // edge pass
    const int e = edge_at[r];
    if (e >= 0 && edge_x[r] >= floor) peak_test(t, c, n, e, c[e - 1], edge_x[r], c[e + 1], 2 * tid);
  }
  // the list's reservation in the row's global list: requested now, used behind the reductions
  __syncthreads();
  const int cnt = s.count;
  if (want_median && tid == 0) s.bc_i = atomicAdd(&a.gcount[row], cnt <= kLoc ? cnt : kList + 1);   // LDS overflow poisons the list
  // ---- one reduction for everything: wavefront shuffles, one LDS hop, lane 0 merges the four wavefronts ----
  double vmax = t.vmax, vmin = t.vmin, hb = t.hb;
  int imax = t.imax < 0 ? -1 : t.imax + 2 * tid, mb = t.mb < 0 ? -1 : t.mb + 2 * tid;
  double sums[5] = {t.s1, t.s2, t.a1, t.a2, double(t.below)};   // (counts < 2^31 are exact in fp64)
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_down(vmax, o, 64);
    const int oi = __shfl_down(imax, o, 64);
    if (oi >= 0 && (imax < 0 || arg_better<0>(ov, oi, vmax, imax))) { vmax = ov; imax = oi; }
    const double hv = __shfl_down(hb, o, 64);
    const int hi_ = __shfl_down(mb, o, 64);
    if (hi_ >= 0 && (mb < 0 || arg_better<2>(hv, hi_, hb, mb))) { hb = hv; mb = hi_; }
    vmin = fmin(vmin, __shfl_down(vmin, o, 64));
#pragma unroll
    for (int q = 0; q < 5; ++q) sums[q] += __shfl_down(sums[q], o, 64);
  }
  if (lane == 0) {
    StreamWave& w = s.wave[tid >> 6];
    w.vmax = vmax; w.vmin = vmin; w.hb = hb; w.imax = imax; w.mb = mb;
#pragma unroll
    for (int q = 0; q < 5; ++q) w.sums[q] = sums[q];
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < kNWS; ++k) {
      const StreamWave& w = s.wave[k];
      if (w.imax >= 0 && (imax < 0 || arg_better<0>(w.vmax, w.imax, vmax, imax))) { vmax = w.vmax; imax = w.imax; }
      if (w.mb >= 0 && (mb < 0 || arg_better<2>(w.hb, w.mb, hb, mb))) { hb = w.hb; mb = w.mb; }
      vmin = fmin(vmin, w.vmin);
#pragma unroll
      for (int q = 0; q < 5; ++q) sums[q] += w.sums[q];
    }
  }

  // ---- publish: the segment's bracket values join the row's list (one global atomic), its statistics its slot ----
  if (want_median) {
    const int at = s.bc_i;                                     // (written before the reductions' barriers)
    double* dst = a.glist + size_t(row) * kList;
    if (cnt <= kLoc && at >= 0 && at + cnt <= kList)
      for (int k = tid; k < cnt; k += kTS) dst[at + k] = s.list[k];
  }
  if (tid == 0) {
    Partial pt;
    pt.vmax = vmax; pt.vmin = vmin; pt.hb = hb; pt.s1 = sums[0]; pt.s2 = sums[1]; pt.a1 = sums[2]; pt.a2 = sums[3];
    pt.below = (long long)sums[4]; pt.imax = imax; pt.has_min = vmin < INFINITY; pt.mb = mb; pt.pad = 0;
    pt.plat = -INFINITY;
    pt.pfloor = -INFINITY;                                     // (the row's bounds come from the pivot launch on this path)
    a.parts[size_t(row) * S + seg] = pt;
  }
}

// ------------------------------------------------------------------ kernel 3: finish
// One workgroup per row.  finish_row (below) is a sequence of steps; the steps come first.  Every step contains barriers
// (or loops whose trip count is the same for every lane around them) and is called from workgroup-uniform control flow.

struct RowStats {                        // one row's merged segments; every lane holds the same values
  double vmax, vmin;                     // np.max, np.min
  int imax;                              // np.argmax
  double hb;                             // the highest local maximum ...
  int mb;                                // ... and its position (-1: none)
  double s1, s2, a1, a2;                 // the shifted sums of Partial
  long long below;                       // samples under the lower pivot
  double plat;                           // highest reported sample with an equal neighbour (-inf: none)
  double pfloor;                         // highest bound under which samples were left without a peak test (-inf: none)
};

// Step 1 - merge the row's segments; contains barriers.  `sparts` (LDS, kMaxStaged entries) receives the segments'
// results when `staged`: one round of loads, where a loop of global loads over sixteen column blocks costs sixteen
// dependent round trips in this latency-bound launch.  Few segments: every lane runs the same loop, no broadcast needed.
// Many column blocks (row lengths N2 up to 8192: 133 of them): one segment per lane, workgroup reductions.  Both forms
// yield the same values (the sums in their own order each).
template <bool LOCAL>
__device__ __forceinline__ RowStats merge_segments(const PeakArgs& a, int row, const double* c, Shared& s, Partial* sparts, bool staged,
                                                   double pfloor0, int tid) {
  const int S = a.splits, n = a.n;
  RowStats r{};
  r.imax = r.mb = -1;
  r.plat = -INFINITY;
  r.pfloor = pfloor0;
  if (staged) {
    const double* src = reinterpret_cast<const double*>(a.parts + size_t(row) * S);
    double* dst = reinterpret_cast<double*>(sparts);
    for (int i = tid; i < S * int(sizeof(Partial) / sizeof(double)); i += kT) dst[i] = src[i];
    __syncthreads();
  }
  if (LOCAL && staged && S > 16) {
    Partial pt{};                                              // (a lane without a segment: neutral in every reduction)
    pt.imax = pt.mb = -1;
    pt.vmin = INFINITY; pt.plat = pt.pfloor = -INFINITY;
    if (tid < S) pt = sparts[tid];
    r.vmax = pt.vmax; r.imax = pt.imax;
    barg<0>(r.vmax, r.imax, s, tid);
    __syncthreads();
    r.hb = pt.hb; r.mb = pt.mb;
    barg<2>(r.hb, r.mb, s, tid);
    __syncthreads();
    r.vmin = -block_max<kNW>(tid < S && pt.has_min ? -pt.vmin : -INFINITY, s.red_d, tid);
    __syncthreads();
    r.plat = block_max<kNW>(pt.plat, s.red_d, tid);
    __syncthreads();
    r.pfloor = block_max<kNW>(pt.pfloor, s.red_d, tid);
    __syncthreads();
    double sums[4] = {pt.s1, pt.s2, pt.a1, pt.a2};
    bsum_many<4, kNW>(sums, s.many, tid);
    r.s1 = sums[0]; r.s2 = sums[1]; r.a1 = sums[2]; r.a2 = sums[3];
    __syncthreads();
  } else {
    bool has_min = false;
    for (int q = 0; q < S; ++q) {
      const Partial pt = staged ? sparts[q] : a.parts[size_t(row) * S + q];
      r.plat = fmax(r.plat, pt.plat);
      if (pt.imax >= 0 && (r.imax < 0 || arg_better<0>(pt.vmax, pt.imax, r.vmax, r.imax))) { r.vmax = pt.vmax; r.imax = pt.imax; }
      if (pt.has_min && (!has_min || pt.vmin < r.vmin)) { r.vmin = pt.vmin; has_min = true; }
      if (pt.mb >= 0 && (r.mb < 0 || higher(pt.hb, pt.mb, r.hb, r.mb))) { r.hb = pt.hb; r.mb = pt.mb; }
      r.s1 += pt.s1; r.s2 += pt.s2; r.a1 += pt.a1; r.a2 += pt.a2;
      r.below += pt.below;
      if (LOCAL) r.pfloor = fmax(r.pfloor, pt.pfloor);
    }
  }
  if (r.imax < 0) {                                            // no sample reached the pivot launch's bound for the maximum (insurance): scan
    double bv = 0;
    int bi = -1;
    for (int i = tid; i < n; i += kT) {
      const double x = c[i];
      if (x == x && (bi < 0 || x > bv)) { bv = x; bi = i; }
    }
    barg<0>(bv, bi, s, tid);
    if (bi >= 0) { r.vmax = bv; r.imax = bi; }
  }
  if (r.imax < 0 || r.imax >= n) r.imax = 0;                   // all-NaN row (and a guard for every index used below)
  if (r.mb >= n) r.mb = -1;
  return r;
}

// Row test of sample m from memory, for passes that meet every sample of a stretch once: a strict peak, or the START of
// a plateau (which walks to the plateau's end once), becomes the best peak (bh, bm) if it outranks it; `tie` keeps the
// highest tested sample with an equal neighbour.
__device__ __forceinline__ void row_test(const double* c, int n, int m, double& bh, int& bm, double& tie) {
  if (m < 1 || m > n - 2) return;
  const double xl = c[m - 1], x = c[m], xr = c[m + 1];
  if (xl == x || xr == x) tie = fmax(tie, x);
  int at = -1;
  if (xl < x && xr < x) at = m;
  else if (xl < x && xr == x) plateau_mid(c, n, m, x, at);
  if (at >= 0 && (bm < 0 || higher(x, at, bh, bm))) { bh = x; bm = at; }
}

// Step 2 - repair the best peak (r.hb, r.mb) where the segments could not settle it; contains barriers.  Three stages:
// the edge columns of the prime-factor grid, column blocks whose bound lies above the best peak, the whole row.
template <bool LOCAL>
__device__ __forceinline__ void repair_best_peak(const PeakArgs& a, int row, const double* c, Shared& s, const Partial* sparts, bool staged,
                                                 RowStats& r, int tid) {
  const int S = a.splits, n = a.n;
  double tie = -INFINITY;
  double eh = 0;
  int em = -1;
  auto better = [&]() {                                        // the stage's best peak against the row's; the stage's ties join `plat`
    barg<2>(eh, em, s, tid);
    if (em >= 0 && (r.mb < 0 || higher(eh, em, r.hb, r.mb))) { r.hb = eh; r.mb = em; }
    r.plat = fmax(r.plat, block_max<kNW>(tie, s.red_d, tid));
  };
  if (a.edge_n2 > 0) {
    // The segments were column blocks of the prime-factor grid (pfa_cols_stats.h): the samples of the grid's first
    // and last column (neighbours in another output row) had no peak test there, and samples with an equal neighbour
    // were only reported (`plat`; a plateau start that is not in an edge column has been reported).
    const int N2 = a.edge_n2, N1 = n / N2;
    for (int k = tid; k < 2 * N1; k += kT) row_test(c, n, k < N1 ? N2 * k : N2 * (k - N1) + N2 - 1, eh, em, tie);
    better();
  }
  if constexpr (LOCAL) {
    // A column block tested only its samples at or above 0.8 x ITS maximum.  Where that maximum is no peak at all (an
    // end point of the row, or a sample beside a higher one in the next block) and the row's best peak so far is
    // lower than the block's bound, the block's untested samples may hold a higher peak: test that block again, all of
    // it (62 columns x N1 output indices; about one row in a hundred - e.g. the zero-lag maximum of two microphones
    // with equal delays sits at index 0, which is never a peak).
    const int N2 = a.edge_n2, N1 = N2 > 0 ? n / N2 : 0;
    for (int q = 0; q < S && N2 > 0; ++q) {
      const double pf = staged ? sparts[q].pfloor : a.parts[size_t(row) * S + q].pfloor;
      if (!(pf > -INFINITY) || (r.mb >= 0 && r.hb >= pf)) continue;        // (uniform)
      const int c0 = int((long long)q * N2 / S), cols = int((long long)(q + 1) * N2 / S) - c0;   // (the columns are dealt evenly)
      eh = 0;
      em = -1;
      for (int k = tid; k < cols * N1; k += kT) row_test(c, n, c0 + k % cols + N2 * (k / cols), eh, em, tie);
      better();
    }
  }
  // Rescan the row when a reported plateau may outrank the best strict peak, or (separate launches) when the best peak
  // ends up below the pivot launch's bound (the segments only tested samples above it: then it was not a bound -
  // cannot happen while the bound is a value of the row itself, kept as insurance)
  if ((r.plat > -INFINITY && (r.mb < 0 || r.plat >= r.hb)) || (!LOCAL && r.pfloor > -INFINITY && (r.mb < 0 || r.hb < r.pfloor))) {
    eh = 0;
    em = -1;
    for (int m = 1 + tid; m <= n - 2; m += kT) row_test(c, n, m, eh, em, tie);
    barg<2>(eh, em, s, tid);
    r.hb = eh;
    r.mb = em;
  }
}

// Step 3 - SNR (utils.py:238-250): the row's totals minus the window around the maximum; contains barriers
__device__ __forceinline__ double row_snr(const PeakArgs& a, const double* c, Shared& s, const RowStats& r, double k0, int tid) {
  const int n = a.n;
  const int wlo_s = r.imax - a.snr_w > 0 ? r.imax - a.snr_w : 0;
  const int whi_s = r.imax + a.snr_w < n ? r.imax + a.snr_w : n;
  double w1 = 0, w2 = 0;
  for (int i = wlo_s + tid; i < whi_s; i += kT) {
    const double d = c[i] - k0;
    w1 += d;
    w2 += d * d;
  }
  double wsum[2] = {w1, w2};
  bsum_many<2, kNW>(wsum, s.many, tid);
  w1 = wsum[0];
  w2 = wsum[1];
  const double nn = double(n - (whi_s - wlo_s));
  double o1 = r.s1 - w1, o2 = r.s2 - w2;
  if (!(o2 >= 0.25 * r.s2) || nn == 1.0) {
    // the window holds most of the row's energy (strongly correlated signals: a near-delta sequence), so
    // "total minus window" would cancel: sum the noise region itself in one more pass
    // (two passes like np.std: the sample mean k0 may sit 1e3 noise sigmas away when it caught the peak).
    // A noise region of ONE sample (n = 2, 3) goes the same way: its deviation is exactly 0 and the SNR infinite, as
    // np.std gives it; the difference of the one-pass sums leaves a rounding residue there
    double q1 = 0, q2 = 0;
    for (int i = tid; i < n; i += kT)
      if (i < wlo_s || i >= whi_s) q1 += c[i];
    const double mu = bsum(q1, s, tid) / nn;
    for (int i = tid; i < n; i += kT)
      if (i < wlo_s || i >= whi_s) { const double d = c[i] - mu; q2 += d * d; }
    o1 = 0;
    o2 = bsum(q2, s, tid);
  }
  double var = (o2 - o1 * o1 / nn) / nn;
  if (var < 0) var = 0;
  const double noise = sqrt(var);
  return noise == 0.0 ? INFINITY : r.vmax / noise;
}

struct MedianBins {                      // where the fused column pass's histograms place the median of |corr|
  bool have;                             // false: the windows did not overlap around the median - the exact search decides
  unsigned rin1, rin2;                   // ranks of the median's one or two order statistics inside their bins
  double b1lo, b1hi, b2lo, b2hi;         // those bins: [lo, hi)
};

// Step 4 (fused column pass only) - the bins that hold the median's order statistics r1 <= r2; contains barriers.
// Every segment published the counts of 48 histogram bins around its own median and the count below them.  Where
// the windows overlap the sums are the row's exact counts: the bin that holds rank r is a rigorous interval for
// that order statistic (relative width 2^(1/128) - 1 = 0.5 %).
__device__ __forceinline__ MedianBins median_interval(const PeakArgs& a, int row, Shared& s, unsigned r1, unsigned r2, int tid) {
  const int S = a.splits;
  MedianBins m{};
  const BlockHist* bh = a.bh + size_t(row) * S;
  // headers first (one lane per segment), then every (segment, bin) entry by its own lane: two rounds of loads
  __shared__ int swin0[kMaxStaged];
  if (tid < 2 * kWin) s.hist[tid] = 0;                         // [0, kWin): merged bins of the common window; [kWin]: count below it; [kWin + 1]: total
  if (tid < S && tid < kMaxStaged) swin0[tid] = bh[tid].win0;
  __syncthreads();
  int w0 = 0, w1 = kLogBins;
  for (int q = 0; q < S && q < kMaxStaged; ++q) {
    const int v = swin0[q];
    w0 = v > w0 ? v : w0;
    w1 = v + kWin < w1 ? v + kWin : w1;
  }
  if (S > kMaxStaged) w1 = w0;                                 // (guard: more segments than staged - the exact select decides)
  if (tid < S && tid < kMaxStaged) {
    atomicAdd(&s.hist[kWin], bh[tid].below);
    atomicAdd(&s.hist[kWin + 1], bh[tid].total);
  }
  for (int e = tid; e < S * kWin && S <= kMaxStaged; e += kT) {
    const int q = e / kWin, k = e - q * kWin;
    const int b = swin0[q] + k;
    const unsigned v = bh[q].h[k];
    if (b < w0) atomicAdd(&s.hist[kWin], v);
    else if (b < w1) atomicAdd(&s.hist[b - w0], v);
  }
  __syncthreads();
  const unsigned total = s.hist[kWin + 1];
  const unsigned base = s.hist[kWin];
  m.have = w0 < w1 && total == unsigned(a.n) && r1 >= base;
  if (m.have) {
    unsigned e = base;
    int f1 = -1, f2 = -1;
    for (int k = 0; k < w1 - w0; ++k) {
      const unsigned v = s.hist[k];
      if (f1 < 0 && r1 < e + v) { f1 = k; m.rin1 = r1 - e; }
      if (f2 < 0 && r2 < e + v) { f2 = k; m.rin2 = r2 - e; }
      e += v;
    }
    m.have = f1 >= 0 && f2 >= 0;
    if (m.have) {
      m.b1lo = log_bin_floor(w0 + f1); m.b1hi = log_bin_floor(w0 + f1 + 1);
      m.b2lo = log_bin_floor(w0 + f2); m.b2hi = log_bin_floor(w0 + f2 + 1);
    }
  }
  __syncthreads();
  return m;
}

// Step 5 - the exact primary threshold (utils.py:144-149); contains barriers.  mean + std of |corr|, or mult x np.median
// (|corr|): the median from the three launches' bracket list, or - fused column pass - from one pass over the stored row
// for each bin that holds it; the radix select where pivots / windows missed or a list overflowed.
template <bool LOCAL>
__device__ __forceinline__ double exact_threshold(const PeakArgs& a, int row, const double* c, Shared& s, const RowStats& r, const RowPre& pre,
                                                  const MedianBins& mbins, unsigned r1, unsigned r2, int* status, int tid) {
  const int n = a.n;
  if (a.method != 0) {
    double va = (r.a2 - r.a1 * r.a1 / double(n)) / double(n);
    if (va < 0) va = 0;
    return a.mult * ((pre.ka + r.a1 / double(n)) + sqrt(va));          // utils.py:147
  }
  double m0 = 0, m1 = 0;
  bool ok = false;
  if constexpr (LOCAL) {
    if (mbins.have) {
      ok = interval_select(s, tid, c, n, mbins.b1lo, mbins.b1hi, mbins.rin1, m0);
      if (ok) { m1 = m0; if (r2 != r1) ok = interval_select(s, tid, c, n, mbins.b2lo, mbins.b2hi, mbins.rin2, m1); }
    }
    if (tid == 0) atomicAdd(status + (ok ? kStExactMedian : kStRadixFallback), 1);       // diagnostics: rows that needed the exact median / the radix select
  } else {
    const int cnt = a.gcount[row];
    const double* list = a.glist + size_t(row) * kList;
    ok = cnt >= 0 && cnt <= kList && (long long)r1 >= r.below && (long long)r2 < r.below + cnt;
    if (ok) ok = list_select(s, tid, list, cnt, unsigned(r1 - r.below), pre.lo, pre.hi, m0);
    if (ok) { m1 = m0; if (r2 != r1) ok = list_select(s, tid, list, cnt, unsigned(r2 - r.below), pre.lo, pre.hi, m1); }
    if (!ok && tid == 0) atomicAdd(status + kStRadixFallback, 1);           // diagnostics: rows that needed the slow exact select
  }
  if (!ok) {                                                   // exact radix select
    m0 = radix_select(c, n, tid, s, r1);
    m1 = r2 != r1 ? radix_select(c, n, tid, s, r2) : m0;
  }
  return a.mult * (r2 != r1 ? (m0 + m1) * 0.5 : m0);           // np.median = the middle value, or the mean of the two middle ones
}

// np.mean(np.abs(corr)) (utils.py:155), the alternative threshold of the fallback chain, summed from the stored row
// unless `have` it already; contains barriers
__device__ __forceinline__ void need_mean_abs(const double* c, int n, Shared& s, int tid, double& mean_abs, bool& have) {
  if (have) return;
  double acc = 0;
  for (int i = tid; i < n; i += kT) acc += fabs(c[i]);
  mean_abs = bsum(acc, s, tid) / double(n);
  __syncthreads();
  have = true;
}

struct Chosen {                          // outcome of the fallback chain; the selected peaks are in s.sel_pos / s.sel_h
  int branch, count;                     // PAL_BR_* bits; peaks selected
  bool overflow, argmax_fallback;        // the distance rule gave up; the chain ended at the row's maximum
};

// Step 6 - the fallback chain (utils.py:152-179) with the primary threshold known to lie in [tlo, thi]; contains barriers.
// Returns false when a comparison fell inside the interval (never when tlo == thi): the caller makes the threshold exact
// and runs the chain again.
__device__ __forceinline__ bool fallback_chain(const SelArgs sa, const double* c, int tid, Shared& s, const RowStats& r, double tlo, double thi,
                                               bool windowed, int wlo, int whi, double& mean_abs, bool& have_mean_abs, Chosen& out) {
  out = Chosen{};
  bool alt = true;                                             // the search runs with mean(|corr|) instead of the primary threshold
  if (r.mb >= 0) {
    if (r.hb >= thi) alt = false;
    else if (r.hb >= tlo) return false;
  }
  if (alt) {                                                   // no peak reaches the primary threshold
    out.branch |= PAL_BR_ALT_THRESHOLD;
    need_mean_abs(c, sa.n, s, tid, mean_abs, have_mean_abs);
    if (!(r.mb >= 0 && r.hb >= mean_abs)) {
      out.branch |= PAL_BR_ARGMAX_NO_PEAKS;
      out.argmax_fallback = true;
      return true;
    }
  }
  const bool first_ok = !windowed;                             // unwindowed: the best peak is already known
  out.count = select_peaks(sa, c, tid, s, alt ? mean_abs : tlo, alt ? mean_abs : thi, windowed, wlo, whi, first_ok ? r.hb : 0.0,
                           first_ok ? r.mb : -1);
  if (out.count == -2) return false;
  if (out.count < 0) out.overflow = true;
  if (out.count == 0 && windowed) {
    out.branch |= PAL_BR_WINDOW_RETRY;
    need_mean_abs(c, sa.n, s, tid, mean_abs, have_mean_abs);
    out.count = select_peaks(sa, c, tid, s, mean_abs, mean_abs, true, wlo, whi, 0.0, -1);
    if (out.count < 0) out.overflow = true;
    if (out.count == 0) { out.branch |= PAL_BR_ARGMAX_WINDOW; out.argmax_fallback = true; }
  }
  return true;
}

template <bool LOCAL>   // LOCAL: the segments are column blocks of the fused column pass (histogram windows, no pivots)
__device__ __forceinline__ void finish_row(const PeakArgs& a, pal_pair_record* table, int32_t* ksel_multi, double* hsel_multi, int* status, const int row) {
  __shared__ Shared s;
  __shared__ Partial sparts[kMaxStaged];
  const int tid = threadIdx.x;
  const double* c = a.corr + size_t(row) * a.stride;
  const int n = a.n;
  const bool want_median = a.method == 0;
  RowPre pre;                                                  // fused column pass: zero shifts, no row parameters
  if (LOCAL) { pre.k0 = pre.ka = 0; pre.lo = 0; pre.hi = INFINITY; pre.vfloor = pre.pfloor = -INFINITY; }
  else pre = load_pre(a.pre, row);
  const unsigned r1 = unsigned((n - 1) / 2), r2 = unsigned(n / 2);   // ranks of the median's one or two order statistics

  const bool staged = a.splits <= kMaxStaged;
  RowStats r = merge_segments<LOCAL>(a, row, c, s, sparts, staged, pre.pfloor, tid);
  repair_best_peak<LOCAL>(a, row, c, s, sparts, staged, r, tid);
  const double snr = row_snr(a, c, s, r, pre.k0, tid);

  if (a.method < 0) {                                          // metrics only (pal_corr_metrics)
    if (tid == 0) {
      pal_pair_record rec;
      rec.k_sel = r.imax; rec.branch = 0; rec.k_argmax = r.imax; rec.n_sel = 0;
      rec.cmax = r.vmax; rec.cmin = r.vmin; rec.snr = snr; rec.sel_height = r.vmax;
      table[row] = rec;
    }
    return;
  }

  // ---- primary threshold: exact from the start, or (fused column pass, median) an interval [tlo, thi] that holds it ----
  MedianBins mbins{};
  if constexpr (LOCAL) {
    if (want_median) mbins = median_interval(a, row, s, r1, r2, tid);
  }
  double tlo = 0, thi = 0;
  if (mbins.have) {                                            // np.median = the middle value, or the mean of the two middle ones
    const double ml = r2 != r1 ? (mbins.b1lo + mbins.b2lo) * 0.5 : mbins.b1lo, mh = r2 != r1 ? (mbins.b1hi + mbins.b2hi) * 0.5 : mbins.b1hi;
    tlo = a.mult >= 0 ? a.mult * ml : a.mult * mh;
    thi = a.mult >= 0 ? a.mult * mh : a.mult * ml;
  }
  const bool windowed = !isnan(a.med);
  int wlo = 1, whi = n - 2;
  if (windowed) {
    const double span = a.med * a.fs;
    const double c0 = double(a.n2 - 1);
    const double flo = c0 - span - 2.0, fhi = c0 + span + 2.0;
    wlo = flo > 1.0 ? (flo < double(n) ? int(flo) : n) : 1;
    whi = fhi < double(n - 2) ? (fhi > -1.0 ? int(fhi) : -1) : n - 2;
  }
  const SelArgs sa{n, a.n2, a.dist, a.num_peaks, a.fs, a.med, a.bits ? a.bits + size_t(row) * 2 * ((n + 31) / 32) : nullptr, a.memo_cap, a.stack_cap};
  // The fused column pass sums |x| only for the 'adaptive' method; the (rare) fallback branches sum it from the stored row.
  double mean_abs = pre.ka + r.a1 / double(n);
  bool have_mean_abs = !(LOCAL && want_median);

  // ---- fallback chain: on the interval first, where there is one; a comparison inside it sends the row through a
  //      second round with the exact threshold.  Without an interval the first round is exact, and final. ----
  const int exact_round = mbins.have ? 1 : 0;
  Chosen ch;
  for (int round = 0; round < 2; ++round) {
    if (round == exact_round) tlo = thi = exact_threshold<LOCAL>(a, row, c, s, r, pre, mbins, r1, r2, status, tid);
    if (fallback_chain(sa, c, tid, s, r, tlo, thi, windowed, wlo, whi, mean_abs, have_mean_abs, ch)) break;
  }
  if (ch.argmax_fallback || ch.overflow) {
    if (tid == 0) { s.sel_pos[0] = r.imax; s.sel_h[0] = r.vmax; }
    ch.count = 1;
  }

  if (tid == 0) {
    pal_pair_record rec;
    rec.k_sel = s.sel_pos[0];
    rec.branch = ch.branch;
    rec.k_argmax = r.imax;
    rec.n_sel = ch.count;
    rec.cmax = r.vmax;
    rec.cmin = r.vmin;
    rec.snr = snr;
    rec.sel_height = s.sel_h[0];
    table[row] = rec;
    if (ksel_multi)
      for (int k = 0; k < PAL_MAX_PEAKS; ++k) ksel_multi[size_t(row) * PAL_MAX_PEAKS + k] = k < ch.count ? s.sel_pos[k] : -1;
    if (hsel_multi)                                            // heights of the selected peaks only: the reader goes by ksel_multi
      for (int k = 0; k < ch.count; ++k) hsel_multi[size_t(row) * PAL_MAX_PEAKS + k] = s.sel_h[k];
    if (ch.overflow) atomicOr(status + kStOverflow, 1);
  }
}

template <bool LOCAL>
__global__ __launch_bounds__(kT, 4) void k_peak_finish(PeakArgs a, pal_pair_record* table, int32_t* ksel_multi, double* hsel_multi, int* status) {   // (4 waves per SIMD = two workgroups per CU: the launch is latency-bound)
  finish_row<LOCAL>(a, table, ksel_multi, hsel_multi, status, blockIdx.x);
}

}  // namespace

// ------------------------------------------------------------------ host entry points
int Engine::peaks_setup(const double* corr, size_t stride, int rows, int n, int n2, const pal_phat_params& prm, int blocks, int grid_n2,
                        int slot, PeakArgs& a) {
  const bool metrics_only = prm.threshold_method < 0;
  if (!metrics_only) {
    if (prm.num_peaks < 1 || prm.num_peaks > PAL_MAX_PEAKS) return fail(PAL_ERR_INVALID, "num_peaks %d outside 1..%d", prm.num_peaks, PAL_MAX_PEAKS);
    if (prm.peak_distance < 1) return fail(PAL_ERR_INVALID, "`distance` must be greater or equal to 1");
  }
  if (n < 1) return fail(PAL_ERR_INVALID, "empty correlation");
  a.corr = corr; a.stride = stride; a.n = n; a.n2 = n2;
  a.fs = prm.fs; a.mult = prm.threshold_multiplier; a.med = prm.max_expected_delay;
  a.method = prm.threshold_method; a.dist = prm.peak_distance; a.num_peaks = prm.num_peaks;
  const int w = int(0.01 * double(n));                       // utils.py:244
  a.snr_w = w > 1 ? w : 1;
  a.edge_n2 = blocks > 0 ? grid_n2 : 0;
  if (blocks > 0) {
    a.splits = blocks;
    a.tiles_per_seg = 0;
  } else {
    // segments: about 1024 workgroups per launch (four resident per CU, all in flight at once), so that a workgroup
    // streams as many tiles as possible behind one set of fixed costs (row parameters, reductions, publish)
    const int ntiles = ((n + 1) / 2 + kTile - 1) / kTile;
    int want = 1024 / rows;                                     // (rounded down: one resident round rather than a second, short one)
    want = want < 1 ? 1 : (want > ntiles ? ntiles : want);
    a.tiles_per_seg = (ntiles + want - 1) / want;
    if (a.tiles_per_seg > kMaxTilesPerSeg) a.tiles_per_seg = kMaxTilesPerSeg;   // the segment's bracket values must fit its LDS list
    a.splits = (ntiles + a.tiles_per_seg - 1) / a.tiles_per_seg;
  }
  // per-stream scratch: [gcount | pre | parts | glist]; the pivot launch zeroes the list fills
  size_t off_pre = (size_t(rows) * sizeof(int) + 127) & ~size_t(127);
  size_t off_parts = (off_pre + size_t(rows) * sizeof(RowPre) + 127) & ~size_t(127);
  size_t off_list = (off_parts + size_t(rows) * a.splits * sizeof(Partial) + 127) & ~size_t(127);
  // (fused column pass: the segments' histogram windows take the place of the bracket lists)
  const size_t list_bytes = blocks > 0 ? size_t(rows) * a.splits * sizeof(BlockHist) : (a.method == 0 ? size_t(rows) * kList * sizeof(double) : 0);
  const size_t off_bits = (off_list + list_bytes + 127) & ~size_t(127);
  const size_t total = off_bits + (corr ? size_t(rows) * 2 * ((size_t(n) + 31) / 32) * sizeof(unsigned) : 0);   // (bitmaps only where rows are stored)
  char* base = nullptr;
  PAL_TRY(scratch(peak_scratch_slot(slot), total, &base));
  a.gcount = reinterpret_cast<int*>(base);
  a.pre = reinterpret_cast<RowPre*>(base + off_pre);
  a.parts = reinterpret_cast<Partial*>(base + off_parts);
  a.glist = reinterpret_cast<double*>(base + off_list);
  a.bh = reinterpret_cast<BlockHist*>(base + off_list);
  a.bits = corr ? reinterpret_cast<unsigned*>(base + off_bits) : nullptr;
  {
    const int dbg = debug_memo;                                // (PAL_DEBUG_MEMO, tests: a tiny memo sends every chain to the slow path)
    a.memo_cap = dbg > 0 && dbg < kMemo ? dbg : kMemo;
    a.stack_cap = dbg > 0 && dbg < kStack ? dbg : kStack;
  }
  return PAL_OK;
}

int Engine::peaks_finish(PeakArgs& a, int rows, pal_pair_record* table, int32_t* ksel_multi, int slot, double* hsel_multi) {
  const bool metrics_only = a.method < 0;
  const hipStream_t on = stream_of(slot);
  int* status = nullptr;
  PAL_TRY(status_words(&status));
  {
    ProfScope ps(this, metrics_only ? "k_peak_finish(metrics)" : "k_peak_finish", on);
    if (a.tiles_per_seg == 0) k_peak_finish<true><<<dim3(rows), dim3(kT), 0, on>>>(a, table, ksel_multi, hsel_multi, status);
    else k_peak_finish<false><<<dim3(rows), dim3(kT), 0, on>>>(a, table, ksel_multi, hsel_multi, status);
    PAL_HIP(hipGetLastError());
  }
  return PAL_OK;
}

int Engine::peaks(const double* corr, size_t stride, int rows, int n, int n2, const pal_phat_params& prm,
                  pal_pair_record* table, int32_t* ksel_multi, int slot, double* hsel_multi) {
  if (rows <= 0) return PAL_OK;
  const hipStream_t on = stream_of(slot);
  PeakArgs a;
  PAL_TRY(peaks_setup(corr, stride, rows, n, n2, prm, 0, 0, slot, a));
  {
    ProfScope ps(this, "k_peak_pivots", on);
    k_peak_pivots<<<dim3(rows), dim3(kT), 0, on>>>(a);
    PAL_HIP(hipGetLastError());
  }
  {
    ProfScope ps(this, "k_peak_stream", on);
    k_peak_stream<<<dim3(unsigned(rows) * unsigned(a.splits)), dim3(kTS), 0, on>>>(a);
    PAL_HIP(hipGetLastError());
  }
  return peaks_finish(a, rows, table, ksel_multi, slot, hsel_multi);
}

}  // namespace pal
