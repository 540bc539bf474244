// engine.h - internal C++ state behind the pal_handle of include/pal_hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/pal_hip.h"
#include "fin_scratch.h"
#include "fft_core.h"
#include "pair_route.h"
#include "plan_geometry.h"
#include "peak_types.h"
#include "resample_math.h"

namespace pal {

// One circular convolution of length M = M1 x M2 (four-step): its geometry (plan_geometry.h) and device tables.
struct FinArgs;     // pfa_cols_fin.h

struct Conv {
  ConvGeom g;
  cd* chat = nullptr;            // FFT_M of the chirp kernel in [k1][k2] order, pre-scaled
  cd* twA = nullptr;             // exp(-2 pi i q / M1), q < M1
  cd* twB = nullptr;             // exp(-2 pi i r / M),  r < M2
  size_t M() const { return g.m; }
  int M1() const { return g.m1; }
  int M2() const { return 1 << g.l2; }
};

// Prime-factor cut n = N1 x N2 (coprime, both odd) of the inverse PHAT transform (pfa.hip): N2-point DFTs as
// chirp convolutions of length M = 2^lm that never leave LDS, then dense N1-point DFTs down the columns.
struct Pfa : PfaSplit {     // the cut itself (plan_geometry.h: n1, n2, lm, u1, u2, e1, e2, nch, rader, r89) and its device tables
  cd* b = nullptr;         // chirp exp(i pi u2 j^2 / N2), j < N2
  cd* hhat = nullptr;      // FFT_M of the conjugate chirp kernel, scaled by 1 / (M n)
  cd* r1 = nullptr;        // exp(-2 pi i q / N1), q < N1
  double* T = nullptr;     // cos / sin (2 pi j t / N1) in the column pass's chunked order
  int2* rowtab = nullptr;  // per row of Y: (u1 row mod N1, its step between outputs of a last-stage butterfly)
  // `rader`: the Rader variant of the row pass (pfa_rader.h), N2 prime and N2 - 1 = 11 x 9 x 10
  cd *rd_bhat_f = nullptr;   // forward direction (pfa_forward.h): FFT_L of exp(-2 pi i u2 g^s / N2) / L
  cd* rd_bhat = nullptr;     // 3-D spectrum of the Rader kernel sequence in prime-factor positions (mixed_radix.h)
  int *rd_qidx = nullptr, *rd_ridx = nullptr;
  void* r89_tab = nullptr;   // `r89`, N1 = 89: tables of the Rader column transform (pfa_rader89.h: Rader89Tab)
  int rows() const { return (n1 + 1) / 2; }   // spectrum rows k1 <= (N1-1)/2 kept by the permuted layout
  bool on() const { return n1 > 0; }
};

// Exact-length-n DFT plan (Bluestein / chirp-z): forward real -> half spectrum, inverse pairs.
struct Plan {
  int n = 0;        // DFT length
  int H = 0;        // n/2 + 1 bins of the half spectrum
  int lin = 0;      // longest real input of a forward transform
  int nout = 0;     // outputs kept by an inverse transform (n for PHAT, N of 2N for fractional delay)
  cd* w = nullptr;  // chirp exp(i pi j^2 / n), j < n
  Conv fwd;         // forward:  lin inputs -> H outputs
  Conv inv;         // inverse:  n inputs  -> n outputs (two real sequences per complex transform)
  Pfa pfa;          // prime-factor route of the PHAT inverse when n splits (otherwise `inv` does it)
  long long used = 0;   // Engine::plan_clock at the last get_plan (the cache evicts the least recently used plan)
  // elements per row of the spectra that forward_spectra writes and pair_correlations reads: the half spectrum, or
  // the permuted rows k1 <= (N1-1)/2 of the prime-factor layout
  size_t spec_stride() const { return pfa.on() ? size_t(pfa.rows()) * size_t(pfa.n2) : size_t(H); }
};

struct ProfileSlot {
  double ms = 0;
  int64_t launches = 0;
};

// The engine's growable device scratch blocks (Engine::scratch), by number.  (caller): held by a caller across a call into the pair
// pipeline (pair_correlations and what it launches), which therefore never takes them; it takes the others.
enum Ws : int {
  kWsWork = 0,         // transform workspace of a launch group, one per stream slot (also the forward spectra's and sim.hip's)
  kWsCorr = 1,         // correlation rows of a launch group, one per stream slot (sim.hip: filter / correlation rows)
  kWsSpectra = 2,      // (caller) spectra + non-zero flags of a call's rows: all_pairs_dev, pairs_dev, the bootstrap
  kWsQuads = 3,        // (caller) packed transforms of an explicit pair list (pairs_dev); small tables of sim.hip
  kWsStageIn = 4, kWsStageTable = 5, kWsStageOut = 6, kWsStagePairs = 15,   // (caller) API staging: uploaded rows, records / per-row results, rows out, a pair list
  kWsStatus = 7,       // the status words (peak_types.h StatusWord), see status_words()
  kWsPeaks0 = 8, kWsPeaks1 = 9, kWsPeaks2 = 12,         // peak selection (peaks.hip) per stream slot, see peak_scratch_slot
  kWsBootRows = 10, kWsBootRound = 11, kWsBootPeaks = 13,   // (caller) the bootstrap's shuffled rows, round tables (pair list, transforms, records), host-call peaks
  kWsZeroRows = 14,    // per row of a call: a microphone of the pair is silent (k_pair_zero)
  kWsFin0 = 16, kWsFin1 = 17, kWsFin2 = 18,             // the finishing column pass (pfa_cols_fin.h, fin_scratch.h) per stream slot, see fin_scratch_slot
  kWsFlags = 19, kWsFlagQuads = 20, kWsFlagTable = 21,  // its flagged pairs: [flags | list | count], their packed transforms, their repaired records
  kWsSolve = 22,       // the position solve (solve.hip): uploaded small inputs, (b, w) per pair, starts, per-start results, records
  kWsBlockTable = 23,  // (caller) records in blocked pair order (all_pairs_dev, large arrays)
  kWsResample = 24,    // resample.hip: the interleaved (win, delta) filter table of the latest ratio
  kWsClosure = 25,     // the closure check (closure.hip): frame lengths, dense lag matrices, votes when the caller takes none
  kWsFinStrip0 = 26, kWsFinStrip1 = 27, kWsFinStrip2 = 28,   // its SNR strips (pair_route.h fin_strip) per stream slot, see fin_strip_slot
  kWsConsensus = 29,   // the consensus (consensus.hip): frame lengths, candidate cubes, chosen-lag matrices, three selections, two vote tables
  kWsCandK = 30, kWsCandH = 31,   // the selected peaks of a launch group per stream slot (PAL_MAX_PEAKS indices / heights per row), compacted into a CandOut
  kWsSrp = 32,         // SRP (srp.hip): a frame slice's correlation rows and one-peak table (the strips call); microphones, direction tables, clip counters, peak marks, the map when the caller takes none (SrpCarve: every other call)
  kWsBeam = 33,        // the delay-and-sum beamformer (beamform.hip): a frame slice's spectra and row flags, its beam spectra, exponents and live marks; MVDR adds a group's covariance triangle and weights
  kWsCount = 34
};
constexpr Ws peak_scratch_slot(int slot) { return slot == 0 ? kWsPeaks0 : (slot == 1 ? kWsPeaks1 : kWsPeaks2); }
constexpr Ws fin_scratch_slot(int slot) { return Ws(kWsFin0 + slot); }
constexpr Ws fin_strip_slot(int slot) { return Ws(kWsFinStrip0 + slot); }

// One scratch block carved into 256-byte aligned pieces: take(bytes) is the piece's offset, `off` the block's size so far.
struct Carve {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t at = off;
    off = (off + bytes + 255) & ~size_t(255);
    return at;
  }
};

// K = num_peaks candidate peaks per pair of a batched call (pal_gcc_phat_*_peaks*): k[npairs][K] array indices, -1 past n_sel;
// h[npairs][K] heights, +0.0 past n_sel, or nullptr
struct CandOut {
  int32_t* k;
  double* h;
};

struct Engine {
  int device = 0;
  int cu_count = 256;              // compute units of the device (persistent kernels size their grids with it)
  hipStream_t stream = nullptr;    // FFT passes, copies, everything a caller can order against
  hipStream_t stream2 = nullptr;   // second and third launch-group slots (pair_correlations; PAL_OVERLAP=0: `stream` only)
  hipStream_t stream3 = nullptr;
  hipStream_t stream_of(int slot) const { return slot == 0 ? stream : (slot == 1 ? stream2 : stream3); }   // launch-group slot -> its stream
  hipEvent_t ev_fork = nullptr, ev_join2 = nullptr, ev_join3 = nullptr;   // side slots start behind `stream`; `stream` waits for them at the end
  hipEvent_t ev_fin = nullptr;     // end of the latest finishing column pass (pfa_cols_fin.h): they run one at a time, see fin_serialize
  int fin_serialize(hipStream_t on);   // before such a launch: wait for the previous one; fin_done(on) behind it
  int fin_done(hipStream_t on);
  bool fin_pending = false;
  bool fin_serial = false;         // PAL_FIN_SERIAL=1
  // switches of the finishing pass, read when the engine is created (not once per process: tests build engines under
  // different settings)
  bool rows_lean = true;           // PAL_ROWS_LEAN=0: stored rows of the other routes keep the three statistics launches
  long long rows_lean_min = 200000;   // PAL_ROWS_LEAN_MIN=<pairs>: smallest call that takes k_rows_lean (tests lower it)
  bool lean_store = true;          // PAL_LEAN_STORE=0: stored rows keep the round-2 statistics (pfa_cols_stats.h / three launches) + k_peak_finish
  int debug_memo = 0;              // PAL_DEBUG_MEMO=<n>: shrinks the distance rule's on-chip memo / stack (tests of its slow path)
  bool one_stream = false;         // PAL_OVERLAP=0: every launch on `stream` (default: launch groups rotate over three streams)
  PlanSwitches plan_sw;            // PAL_RADIX3, PAL_FOUR_REG, PAL_PFA, PAL_PFA_BIG, PAL_RADER, PAL_R89: what shapes a plan (plan_geometry.h)
  bool xcd_rows = true;            // PAL_XCD_ROWS=0: row passes in plain workgroup order (pfa_kernels.h: row_work_item)
  bool rows_shared = true;         // PAL_ROWS_SHARED=0: the Rader row pass reads all four spectrum rows even when two are the same (pfa_rader.h)
  std::string err;
  static constexpr int kDefaultChunk = 128;
  int chunk = kDefaultChunk;                    // transforms per launch group (forward spectra, simulation, synchronisation)
  bool chunk_auto = true;                       // pair pipeline: 240 transforms per group where a workspace slot stays <= 1 GiB
                                                // (480 rows: the finish launch's workgroups, two per CU, leave slots free
                                                //  beside the other streams' launches - 256 measured 3 % less than 240)
  int pair_group(int n) const {                 // (PAL_CHUNK / pal_set_chunk fix both)
    if (!chunk_auto) return chunk;
    const long long g = (1ll << 30) / (16ll * (n > 0 ? n : 1));
    return int(g < 32 ? 32 : (g > 240 ? 240 : g));
  }
  std::map<std::tuple<int, int, int>, Plan> plans;   // (n, lin, nout) -> plan
  struct XConv { Conv conv; long long used = 0; };
  std::map<size_t, XConv> xconvs;                    // sequence length -> convolution of pal_xcorr_vs_ref
  int max_plans = 64;                                // PAL_MAX_PLANS / pal_set_max_plans: bound of both caches (least recently used out first)
  long long plans_built = 0, plans_evicted = 0;      // pal_plan_stats
  long long plan_clock = 0;
  cd* stage_tw[16] = {};                        // stage-major twiddles per log2 N (<= 14: the big row tiles of pfa_big.h)
  cd* stage_twc[16] = {};                       // the same with a compact last stage (fft_core.h stage_twc_size)
  // growable device scratch
  void* ws[kWsCount] = {};
  size_t ws_bytes[kWsCount] = {};
  // profiling
  bool profiling = false;
  int prof_every = 1;              // pair pipeline: events around every prof_every-th launch group only
  long long prof_tick = 0;
  bool prof_gate = true;           // false while an unsampled launch group is being enqueued
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  struct Pending { int slot; hipEvent_t a, b; };
  std::vector<Pending> pending;
  std::vector<std::string> slot_names;
  std::vector<ProfileSlot> slots;
  // rccl
  void* comm = nullptr;
  // device copy of the (trial, i<j) pair table of the last all-pairs shape
  void* quads = nullptr;
  int quad_B = 0, quad_M = 0;
  // pair blocking (large arrays): pairs processed in 16 x 16 blocks of microphones, records scattered back to row-major order
  int4* quads_blk = nullptr;
  int* perm_blk = nullptr;
  int blk_B = 0, blk_M = 0;
  int pair_block = 16;             // PAL_PAIR_BLOCK=<microphones per block side>, 0 = off; used from 96 microphones up

  int fail(int code, const char* fmt, ...);
  int check(hipError_t e, const char* what);
  int scratch(Ws idx, size_t bytes, void** out);
  template <class T> int scratch(Ws idx, size_t bytes, T** out) {   // the same block as a T*
    void* p = nullptr;
    const int rc = scratch(idx, bytes, &p);
    *out = static_cast<T*>(p);
    return rc;
  }
  int status_words(int** out) { return scratch(kWsStatus, kStatusWords * sizeof(int), out); }   // peak_types.h StatusWord; zeroed when first taken
  int upload_lengths(const int32_t* lengths, int B, void* d_dst);   // a call's frame lengths (host) -> device; the stream is synchronised behind the copy
  const cd* stage_table(int ln, bool compact = false);   // stage_tw[ln] / stage_twc[ln], made on first use (null: out of memory)
  int build_pfa(Plan& pl);                  // pfa.hip: the split of plan_geometry.h and its tables, built in pl.pfa (off if no split fits)
  void free_pfa(Pfa& f);
  int build_rader(Pfa& f, long long n, long long u2);   // pfa.hip: Rader tables when N2 is 991
  int pfa_pair_group(const Plan& pl, const cd* permuted, const int4* quads, int G, cd* Y, double* corr, size_t stride,
                     const int* zero_rows, hipStream_t on);
  int get_plan(int n, int lin, int nout, Plan** out);
  void free_plan(Plan& pl);
  int clear_plans();
  int xcorr_conv(size_t len, Conv** out);
  int alloc_conv(Conv& c, size_t needed);   // geometry, tables and chirp-spectrum storage for >= `needed` points
  void free_conv(Conv& c);
  int build_conv(Conv& c, const cd* w, int n, int neg_count, int pos_count, bool conj_kernel, double extra_scale);
  // profiling helpers
  int prof_slot(const char* name);
  void prof_begin(int slot, hipEvent_t* a, hipStream_t on);
  void prof_end(int slot, hipEvent_t a, hipStream_t on);
  void prof_flush();

  // pipelines (all pointers are device pointers)
  int forward_spectra(Plan& pl, const double* frames, size_t frame_stride, int rows, int len, cd* spectra, int* nonzero = nullptr);
  int pair_correlations(Plan& pl, const cd* spectra, int nspec, const int4* quads, int64_t npairs, int n2,
                        const pal_phat_params& prm, pal_pair_record* table, int32_t* ksel_multi, double* corr_out,
                        const int* nonzero = nullptr, bool stored_only = false,    // stored_only: the repair pass of flagged pairs (pair_route.h)
                        const CandOut* cands = nullptr);                           // cands: K candidate peaks per pair into the caller's buffers
  int pairs_dev(const double* d_rows, int R, int L, const int32_t* d_pairs, int64_t P, const pal_phat_params& prm,
                pal_pair_record* d_table, const CandOut* cands = nullptr);
  // bootstrap.hip: counter-based shuffles (pal_bootstrap_shuffle_dev) and the shuffled pairs through the pair pipeline, round by round
  int bootstrap_shuffle_dev(const double* d_row, int L, int32_t i, int32_t j, int32_t mode, int32_t block_size, uint64_t seed, int64_t s0,
                            int32_t S, double* d_out);
  int bootstrap_round(const Plan& pl, int L) const;   // shuffled rows per round
  int bootstrap_peaks_dev(const double* d_rows, int R, int L, const int32_t* d_pairs, int64_t P, int32_t S, int32_t mode, int32_t block_size,
                          uint64_t seed, double* d_peaks);
  // solve.hip: TDOA tables -> positions (d_tables in HBM, every other argument a host array); returns with `out` filled
  int solve_positions_dev(const pal_pair_record* d_tables, int B, int M, const int32_t* lengths, const double* mics, const double* calib,
                          const double* weights, const double* extra_starts, const pal_solve_params* prm, pal_position_record* out);
  // the same under a robust loss (PAL_SOLVE_LOSS_*, scale f_scale); pair_weights[B][P] (host, or nullptr): rho'(z) of every pair
  int solve_positions_loss_dev(const pal_pair_record* d_tables, int B, int M, const int32_t* lengths, const double* mics, const double* calib,
                               const double* weights, const double* extra_starts, const pal_solve_params* prm, pal_position_record* out,
                               int loss, double f_scale, double* pair_weights);
  int solve_positions_impl(const pal_pair_record* d_tables, int B, int M, const int32_t* lengths, const double* mics, const double* calib,
                           const double* weights, const double* extra_starts, const pal_solve_params* prm, pal_position_record* out,
                           int loss, double f_scale, double* pair_weights);
  // closure.hip: loop closure of TDOA tables (d_tables and the four outputs in HBM, each output or nullptr; lengths a host array); asynchronous
  int tdoa_closure_dev(const pal_pair_record* d_tables, int B, int M, const int32_t* lengths, int32_t tol, int32_t min_votes, int32_t weight_mode,
                       int32_t* d_votes, int32_t* d_mic_closed, double* d_weights, pal_closure_frame* d_summary);
  int closure_check(int B, int M, const int32_t* lengths, int32_t tol, int32_t min_votes, int32_t weight_mode);
  int lag_votes(const int32_t* d_lag, int B, int M, int tol, int32_t* d_votes);   // k_closure_votes on B lag matrices [M][M] -> votes [B][P]
  int frames_check(const char* what, int B, int M, const int32_t* lengths, int32_t tol);   // the checks closure_check and consensus_check share
  // consensus.hip: loop-closure consensus over K candidates per pair (every pointer but `lengths` in HBM, each output or nullptr); asynchronous
  int tdoa_consensus_dev(const pal_pair_record* d_tables, const int32_t* d_cand_k, const double* d_cand_h, int B, int M, int K,
                         const int32_t* lengths, int32_t tol, int32_t rounds, int32_t* d_sel, pal_pair_record* d_table_out,
                         pal_consensus_frame* d_summary);
  int consensus_check(int B, int M, int K, const int32_t* lengths, int32_t tol, int32_t rounds);
  // srp.hip: lag strips of stored rows, the steered-response power map and its peaks (every pointer but `mics` and `grid` in HBM, each
  // output or nullptr); asynchronous.  The *_check functions hold the argument checks that the host and the _dev forms share; the maps'
  // and the zooms' go through one common check of B, M, T, mics, fs, c, K, R and the outputs, the cheap checks first.
  int srp_strips_check(int B, int M, int L, int T, int W);
  int srp_strips_rows(const double* d_rows, int64_t nrows, int L, int T, int W, double* d_strips);   // k_srp_strips on rows[nrows][2L-1]
  int srp_map_check(int B, int M, int T, const double* mics, double fs, double c, const pal_srp_grid* grid, int K, int R, bool any_output,
                    bool peaks_out);
  int srp_map_dev(const double* d_strips, int B, int M, int T, const double* mics, double fs, double c, const pal_srp_grid* grid,
                  const double* d_pair_weights, int K, int R, double* d_power, pal_srp_peak* d_peaks, pal_srp_frame* d_summary);
  int srp_peaks_check(int B, const pal_srp_grid* grid, int K, int R);
  int srp_peaks_dev(const double* d_power, int B, const pal_srp_grid* grid, int K, int R, pal_srp_peak* d_peaks, pal_srp_frame* d_summary);
  // the coarse-to-fine zoom around seeds[B][K] (k_srp_zoom): `mics` and `half0` are host memory
  int srp_zoom_check(int B, int M, int T, const double* mics, double fs, double c, int K, const double* half0, int Z, int levels);
  int srp_zoom_dev(const double* d_strips, int B, int M, int T, const double* mics, double fs, double c, const double* d_pair_weights,
                   const pal_srp_peak* d_seeds, int K, const double* half0, int Z, int levels, pal_srp_zoom_record* d_out);
  // the direction map, its peaks and its zoom (k_srp_doa, k_srp_doa_peaks, k_srp_doa_zoom, also in srp.hip): `mics`, `grid`, `az` and
  // `el` are host memory
  int srp_doa_check(int B, int M, int T, const double* mics, double fs, double c, const pal_srp_doa_grid* grid, const double* az,
                    const double* el, int K, int R, bool any_output, bool peaks_out);
  int srp_doa_dev(const double* d_strips, int B, int M, int T, const double* mics, double fs, double c, const pal_srp_doa_grid* grid,
                  const double* az, const double* el, const double* d_pair_weights, int K, int R, double* d_power, pal_srp_peak* d_peaks,
                  pal_srp_frame* d_summary);
  int srp_doa_peaks_check(int B, const pal_srp_doa_grid* grid, const double* az, const double* el, int K, int R);
  int srp_doa_peaks_dev(const double* d_power, int B, const pal_srp_doa_grid* grid, const double* az, const double* el, int K, int R,
                        pal_srp_peak* d_peaks, pal_srp_frame* d_summary);
  int srp_doa_zoom_check(int B, int M, int T, const double* mics, double fs, double c, int K, double half0, int Z, int levels);
  int srp_doa_zoom_dev(const double* d_strips, int B, int M, int T, const double* mics, double fs, double c, const double* d_pair_weights,
                       const pal_srp_peak* d_seeds, int K, double half0, int Z, int levels, pal_srp_zoom_record* d_out);
  // beamform.hip: delay-and-sum beams of frames[B][M][L] at delays / weights[B][S][M] -> out[B][S][L] (every pointer in HBM); asynchronous,
  // a non-finite sample or a refused table entry is reported by pal_synchronize (kStInputNonFinite, kStInputBadSteer)
  int steer_check(int B, int M, int L, double fs, int S);
  int steer_sum_dev(const double* d_frames, int B, int M, int L, double fs, const double* d_delays, const double* d_weights, int S,
                    double* d_out);
  // the null-steering beams of the same inputs (beamform.py, separate): S <= 8, loading >= 0 and > 0 where S > 1
  int separate_check(int B, int M, int L, double fs, int S, double loading);
  int separate_dev(const double* d_frames, int B, int M, int L, double fs, const double* d_delays, const double* d_gains, int S,
                   double loading, double* d_out);
  int beams_dev(const double* d_frames, int B, int M, int L, double fs, const double* d_delays, const double* d_weights, int S,
                double* d_out, bool solve, double loading);
  // the MVDR beams of the same frames in G groups of B / G (beamform.py, mvdr): delays / gains[G][S][M], weights from each group's
  // covariance; M <= 64, loading > 0; d_weights: NULL or [G][S][M][L + 1] complex
  int mvdr_check(int B, int M, int L, double fs, int G, int S, double loading);
  int mvdr_dev(const double* d_frames, int B, int M, int L, double fs, const double* d_delays, const double* d_gains, int G, int S,
               double loading, double* d_out, double* d_weights);
  int mvdr_tile = 0;               // PAL_MVDR_TILE=44: 4 x 4 microphone pairs per workgroup of k_mvdr_cov (default 8 x 4; the bytes do not depend on it)
  int beam_slice = 0;              // PAL_BEAM_SLICE=<frames>: frames per slice of steer_sum_dev, separate_dev and mvdr_dev (0: as many as keep the slice's spectra near 1 GiB)
  int32_t* solve_idx = nullptr;    // device table pair -> i | j << 16 of the last microphone count
  int solve_idx_M = 0;
  // resample.hip: the right wing of the interpolation filter as pal_resample_set_filter received it, and the ratio whose scaled
  // (win, delta) table sits in kWsResample (0: none yet)
  std::vector<double> rs_win;
  std::vector<ResampleTap> rs_host;   // the table's host copy (source of its upload)
  int rs_num_table = 0;
  double rs_ratio = 0;
  int peaks(const double* corr, size_t stride, int rows, int n, int n2, const pal_phat_params& prm,
            pal_pair_record* table, int32_t* ksel_multi, int slot, double* hsel_multi = nullptr);   // hsel_multi: heights beside ksel_multi's indices
  // the same in pieces, for the column pass that produces the streaming statistics itself (pfa_cols_stats.h):
  // arguments + scratch (segments = `blocks` column blocks of a grid with rows of grid_n2, each with its own pivots),
  // [the caller's fused column launch], the finish launch
  int peaks_setup(const double* corr, size_t stride, int rows, int n, int n2, const pal_phat_params& prm, int blocks, int grid_n2, int slot, PeakArgs& a);
  int peaks_finish(PeakArgs& a, int rows, pal_pair_record* table, int32_t* ksel_multi, int slot, double* hsel_multi = nullptr);
  int pfa_rows(const Plan& pl, const cd* permuted, const int4* quads, int G, cd* Y, hipStream_t on);
  int fin_setup(const Plan& pl, int rows, int nblk, int grid_rows, const pal_phat_params& prm, int n2, pal_pair_record* table,
                int* need, int slot, PeakArgs& a, struct FinArgs& fa, unsigned& nwg, int G);
  int rows_lean_group(const Plan& pl, const double* corr, size_t stride, int G, int rows, const pal_phat_params& prm, int n2,
                      pal_pair_record* table, int* need, int slot);
  int pfa_pair_group_fin(const Plan& pl, const cd* permuted, const int4* quads, int G, int rows, cd* Y, const int* zero_rows,
                         const pal_phat_params& prm, int n2, pal_pair_record* table, int* need, int slot,
                         double* corr = nullptr, size_t stride = 0);
  int pfa_pair_group_fused(const Plan& pl, const cd* permuted, const int4* quads, int G, int rows, cd* Y, double* corr, size_t stride,
                           const int* zero_rows, const pal_phat_params& prm, int n2, pal_pair_record* table, int32_t* ksel_multi, int slot,
                           double* hsel_multi = nullptr);
  bool pfa_forward_applies(const Plan& pl, int len) const;
  int pfa_forward_spectra(Plan& pl, const double* frames, size_t frame_stride, int rows, int len, cd* spectra, const int* flags);
  bool pfa_forward = true;    // PAL_PFA_FWD=0: forward spectra on the four-step route even where the prime-factor cut applies
  bool fin_cols = true;       // PAL_FIN=0: the fused column pass always stores the correlation rows for a finish launch (pfa_cols_stats.h) instead
                              // of finishing the rows itself without storing them (pfa_cols_fin.h: one peak per row, nobody asks for `corr`)
  unsigned fin_epoch[3] = {};   // launches of the finishing column pass per stream slot (pfa_cols_fin.h: validity tag of what its blocks exchange)
  FinKey fin_key[3];            // the layout of the slot's latest launch (fin_scratch.h: another one zeroes the block)
  unsigned fin_wrap = kFinEpochWrap;   // PAL_DEBUG_FIN_WRAP=<n>: the epoch bound (tests of the reset at the wrap)
  bool fin_strip_on = true;     // PAL_FIN_STRIP=0: windowed calls keep the polling form of the per-wavefront statistics (pair_route.h fin_strip)
  int fin_giveup = 0;           // PAL_DEBUG_FIN_GIVEUP=1: every bounded wait of the pass gives up at once (tests of the stored-row repair)
  bool fuse_peaks = true;     // PAL_FUSED=0: separate column pass + pivot / stream launches instead of the fused column pass +
                              // peak statistics (pfa_cols_stats.h) where that applies
};

struct ProfScope {
  Engine* e;
  int slot;
  hipEvent_t a = nullptr;
  hipStream_t on;
  ProfScope(Engine* eng, const char* name, hipStream_t s = nullptr) : e(eng), slot(-1), on(s ? s : eng->stream) {
    if (e->profiling && e->prof_gate) {
      slot = e->prof_slot(name);
      e->prof_begin(slot, &a, on);
    }
  }
  ~ProfScope() {
    if (slot >= 0) e->prof_end(slot, a, on);
  }
};

#define PAL_TRY(expr)                \
  do {                               \
    int _rc = (expr);                \
    if (_rc != PAL_OK) return _rc;   \
  } while (0)

#define PAL_HIP(expr) PAL_TRY(check((expr), #expr))

}  // namespace pal
