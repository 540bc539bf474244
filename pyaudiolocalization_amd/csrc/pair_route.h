// Route of one call of the pair pipeline (Engine::pair_correlations): who transforms a launch group and who computes its rows'
// statistics, from the plan's shape, the call, the parameters and the engine's switches.  Host code only, no HIP headers:
// tests/host/test_pair_route.cpp compiles it alone and checks it against the rules written out as booleans.
#pragma once

namespace pal {

constexpr int kColsOwn = 62;      // columns a workgroup of the fused column pass owns (64 lanes - two border lanes)

struct RouteIn {
  int n, nout; bool split; int n1, n2, nch, lm; bool r89;   // the plan: Plan.n / nout, Pfa.on() and its n1, n2, nch, lm, whether the Rader-89 column tables exist
  bool table, corr, multi; long long npairs;                // the call: wants records / the correlation rows / several peaks per row (ksel_multi)
  bool stored_only;                                         //   the repair pass of flagged pairs: stored rows + k_peak_finish, nothing that flags again
  int num_peaks, threshold_method; double threshold_multiplier;                 // of pal_phat_params
  bool fin_cols, fuse_peaks, lean_store, rows_lean; long long rows_lean_min;    // PAL_FIN, PAL_FUSED, PAL_LEAN_STORE, PAL_ROWS_LEAN, PAL_ROWS_LEAN_MIN
};

// kFinish: row pass + k_pfa_cols_fin (rows never stored); kLeanStore: the same pass storing the rows (k_pfa_cols_lean); kFused: row pass +
// k_pfa_cols_stats + k_peak_finish; kPfa: row pass + k_pfa_cols; kFourStep: the chirp convolution's three passes (conv_kernels.h)
enum class RouteTransform { kFinish, kLeanStore, kFused, kPfa, kFourStep };
// kNone: no table; kPass: the transform's own column pass; kRowsLean: k_rows_lean; kThreeLaunches: k_peak_pivots + k_peak_stream + k_peak_finish
enum class RouteStats { kNone, kPass, kRowsLean, kThreeLaunches };

struct PairRoute {
  RouteTransform transform;
  RouteStats stats;
  // the route writes one flag per pair (1 = resolved at the end of the call from stored rows)
  bool flags_pairs() const { return transform == RouteTransform::kFinish || transform == RouteTransform::kLeanStore || stats == RouteStats::kRowsLean; }
};

// column blocks per transform of the fused / finishing column passes: kColsOwn columns each, four strips of them where the column
// DFTs are short (one chunk, N1 <= 23: the four wavefronts of a workgroup take four neighbouring strips)
inline int fin_blocks(int n2, int nch) { return (n2 + (nch <= 1 ? 4 : 1) * kColsOwn - 1) / ((nch <= 1 ? 4 : 1) * kColsOwn); }

// the threshold needs no histograms: 'adaptive', or 'median' with a multiplier in 0 .. 2 (pfa_cols_fin.h fin_decide bounds the median)
inline bool nohist(int threshold_method, double threshold_multiplier) {
  return threshold_method > 0 || (threshold_multiplier >= 0 && threshold_multiplier <= 2.0);
}

inline PairRoute pair_route(const RouteIn& f) {
  const bool lean_peak = f.fin_cols && !f.stored_only && f.num_peaks == 1 && !f.multi;   // one peak per row (main.py:204), and not the repair pass
  const bool no_hist = nohist(f.threshold_method, f.threshold_multiplier);
  const int nblk = fin_blocks(f.n2, f.nch);
  // the fused column pass applies when one workgroup covers every output index (nch <= 4 chunks of kPfaTC: N1 <= 89)
  if (f.table && f.fuse_peaks && f.split && f.nch >= 1 && f.nch <= 4 && f.n2 >= 3) {
    // The column pass that finishes the rows itself: the caller does not ask for `corr`, and the grid's rows have at least 256 columns.
    // Measured over L = 44100 ... 44299 with the per-wavefront statistics of pfa_fin_lean.h (profiles/r03_c_length_sweep_dense_fin.csv
    // against ..._default.csv): the pass wins with Rader-89 columns (+10 %), with two or four chunks of output indices (+3 ... +12 %, +4 %)
    // and with short columns beside row tiles of up to 8192 points (+8 %); three chunks leave the fourth wavefront idle (-2 %), and
    // beside the 16384-point row tiles it is a wash
    bool cols_ok = f.r89 || (f.nch >= 2 && f.nch <= 4) || (f.nch <= 1 && f.lm <= 13);
    // ... on grids of at least twelve column blocks per transform (N2 >= 683; strips: N2 >= 2729): with fewer, a launch group is one or
    // two rounds of blocks and the pass is the sum of one block's latencies - the stream chain's lengths (n = 24 000 ... 24 500:
    // 59 x 407, seven blocks) ran 534 frames/s with the pass and 579 without
    if (!f.r89 && nblk < 12) cols_ok = false;
    // (five and six chunks, N1 up to 133, are not finished here: the fused pass stops at four.  Tried with five- /
    // six-wavefront blocks: correct, but C5 ran 2.53 against 2.58 M pairs/s with it - 960 blocks are one round of the machine, every
    // wavefront is in the same phase at the same time and the pass (160 us) is the sum of its latencies, where the separate launches
    // (70 + 18 + 31 + 32) overlap.  Their stored rows take k_rows_lean)
    if (lean_peak && !f.corr && f.n2 >= 256 && cols_ok) return {RouteTransform::kFinish, RouteStats::kPass};
    // The same pass with the rows stored as well (the caller wants them, or the plan has no finishing form that pays), where the threshold
    // needs no histograms.  Several rounds of column blocks per launch group, or the pass is the sum of one block's latencies: C5 (103 x 233:
    // four blocks per transform, 960 per group, one round) measured 2.32 against 2.60 M pairs/s with it; C3 (7 x 6857: 28 blocks) 1.16 against
    // 1.08, C2 (17 x 5647: 23 blocks) 0.422 against 0.417
    // (five and six chunks, N1 = 91 ... 127 beside 700 - 970 columns: 0.63 - 0.66 against 0.69 - 0.71 M with it: they keep the three statistics launches)
    if (f.lean_store && lean_peak && nblk >= 12 && no_hist) return {RouteTransform::kLeanStore, RouteStats::kPass};
    return {RouteTransform::kFused, RouteStats::kPass};
  }
  const RouteTransform tr = f.split ? RouteTransform::kPfa : RouteTransform::kFourStep;
  if (!f.table) return {tr, RouteStats::kNone};
  // Stored rows of these routes: one launch (k_rows_lean) instead of pivots + stream + finish where the threshold needs no histograms.
  // Measured: rows of 12 013 ... 24 013 samples +2 ... +8 % (C5 2.58 -> 2.87 M pairs/s: 66 us per group against 18 + 31 + 32), rows of
  // 88 201 ... 88 367 -3 ... +1 %, C4's 191 999 the same: long rows keep the three launches (their stream pass runs at the HBM rate)
  // (calls of at least 200 000 pairs: the end-of-call count and the flagged rows' second pass - 1.8 % of the rows at C5's lag window -
  //  cost the 30 000 - 80 000-pair calls of the stream chain more than the launch saves, and stall its host: 480 - 497 against 527 - 535 frames/s)
  const bool lean = f.rows_lean && lean_peak && f.npairs >= f.rows_lean_min && no_hist && f.nout == f.n && f.n >= 4096 && f.n <= 50000;
  return {tr, lean ? RouteStats::kRowsLean : RouteStats::kThreeLaunches};
}


// ---- the SNR strip of the finishing pass (pfa_fin_lean.h, strip form).  A windowed call says where a row's argmax can be expected,
// so the samples its SNR window [imax - snr_w, imax + snr_w) may need are known before the launch: the wavefronts store them to a
// strip of the scratch, nobody waits for the row's argmax in the middle of the pass, and the finishing wavefront sums the window from
// the strip (a row whose argmax lies elsewhere has its window evaluated from the grid by the definition of the column transform).
// Up to three pieces, with D the window's half width in samples (the lag max_expected_delay):
//     the row's ends   [0, D + snr_w - 1] and [n - D - snr_w, n - 1]: the rows are circular correlations as the inverse transform
//                      leaves them - lag 0 is index 0, a delay of +d samples is index d, of -d samples index n - d.  A source whose
//                      delay the caller's bound allows has its maximum HERE (every row of the metric run does:
//                      tests/golden/metric_44k1_first24.npz), not inside the lag window that the selection searches;
//     the centre       [win_lo - snr_w, win_hi + snr_w - 1]: a row whose maximum is the lag window's own best sample.
// Pieces that touch are merged; all are clipped to the row.
#if defined(__HIPCC__) || defined(__CUDACC__)
#define PAL_ROUTE_HD __host__ __device__
#else
#define PAL_ROUTE_HD
#endif

// The strip pays while it is a small share of the row: every sample of it is one more device-scope store per row, and the wait it
// replaces is a fixed cost per wavefront.  Measured on the metric run, strip form against PAL_FIN_STRIP=0 at the same lag window,
// lines alternating (profiles/fin_strip_runs.txt; M pairs/s, lowest - highest): share 14 % (max_expected_delay 0.05 s) 1.750 - 1.773
// against 1.656 - 1.694, 24 % (0.10 s) 1.703 - 1.709 against 1.620 - 1.640, 34 % (0.15 s) 1.667 - 1.669 against 1.633 - 1.646, 64 %
// (0.30 s) 1.558 - 1.568 against 1.618 - 1.631: the largest share at which the strip form still won
constexpr double kFinStripShare = 0.34;
constexpr int kFinStripPieces = 3;

struct FinStrip {                   // plain data: travels to the kernels inside FinArgs
  int pieces;                       // 0: no strip (the polling form)
  int lo[kFinStripPieces], hi[kFinStripPieces];   // [lo, hi] sample indices, ascending and disjoint; unused pieces are empty (lo 1, hi 0)
  int base[kFinStripPieces];        // offset of lo[p] inside the strip
  int len;                          // samples per row of the strip
  bool on() const { return pieces > 0; }
};

inline FinStrip fin_no_strip() {
  FinStrip s;
  s.pieces = 0;
  s.len = 0;
  for (int p = 0; p < kFinStripPieces; ++p) { s.lo[p] = 1; s.hi[p] = 0; s.base[p] = 0; }
  return s;
}

// `lean_finish`: the route is kFinish with the per-wavefront statistics (no histogram body, rows not stored); `enabled`: PAL_FIN_STRIP
inline FinStrip fin_strip(int n, bool windowed, int win_lo, int win_hi, int snr_w, bool lean_finish, bool enabled) {
  FinStrip s = fin_no_strip();
  if (!enabled || !lean_finish || !windowed || win_lo > win_hi || n < 1 || snr_w < 1) return s;
  const long long D = ((long long)win_hi - win_lo + 1) / 2;   // (the window [c - D, c + D]; clipped at the row's ends it is most of the row anyway)
  long long lo[3] = {0, (long long)win_lo - snr_w, (long long)n - D - snr_w};
  long long hi[3] = {D + snr_w - 1, (long long)win_hi + snr_w - 1, (long long)n - 1};
  long long total = 0;
  for (int p = 0; p < 3; ++p) {
    if (lo[p] < 0) lo[p] = 0;
    if (hi[p] > n - 1) hi[p] = n - 1;
    if (s.pieces > 0 && lo[p] <= (long long)s.hi[s.pieces - 1] + 1) {          // touches the piece before it: one piece
      if (hi[p] > s.hi[s.pieces - 1]) { total += hi[p] - s.hi[s.pieces - 1]; s.hi[s.pieces - 1] = int(hi[p]); }
      continue;
    }
    s.lo[s.pieces] = int(lo[p]);
    s.hi[s.pieces] = int(hi[p]);
    s.base[s.pieces] = int(total);
    total += hi[p] - lo[p] + 1;
    ++s.pieces;
  }
  if (double(total) > kFinStripShare * double(n)) return fin_no_strip();
  s.len = int(total);
  return s;
}

// offset of sample m inside the strip, -1 where the strip does not hold it (the wavefronts store exactly the samples with an offset)
PAL_ROUTE_HD inline int fin_strip_offset(const FinStrip& s, int m) {
  int off = -1;
  for (int p = 0; p < kFinStripPieces; ++p) off = m >= s.lo[p] && m <= s.hi[p] ? s.base[p] + (m - s.lo[p]) : off;
  return off;
}
// the finisher's rule: the SNR window [lo, hi) is summed from the strip iff ONE piece holds all of it (its samples are then
// consecutive in the strip, from the offset returned; -1: evaluate it from the grid) - a matter of the row's argmax alone, never of timing
PAL_ROUTE_HD inline int fin_strip_window(const FinStrip& s, int lo, int hi) {
  int off = -1;
  for (int p = 0; p < kFinStripPieces; ++p) off = lo < hi && lo >= s.lo[p] && hi - 1 <= s.hi[p] ? s.base[p] + (lo - s.lo[p]) : off;
  return off;
}
// the SNR window around a row's argmax (utils.py:238-250), [lo, hi)
PAL_ROUTE_HD inline void fin_snr_window(int imax, int snr_w, int n, int& lo, int& hi) {
  lo = imax - snr_w > 0 ? imax - snr_w : 0;
  hi = imax + snr_w < n ? imax + snr_w : n;
}

}  // namespace pal
