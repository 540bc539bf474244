/* pal_hip.h - C ABI of the MI355X GCC-PHAT / multipath engine (libpal_hip.so).
 *
 * The reference (zeynelacikgoez/PyAudioLocalization) is pure Python and has no FFI of its own;
 * its boundary for this path is the set of module-level functions cited at each entry point
 * below (file:line into the reference).  A maintainer binds these symbols with ctypes - the
 * stub is shown in INTEGRATION.md and shipped as pyaudiolocalization_amd/_ffi.py.
 *
 * Conventions
 *   - every call returns 0 (PAL_OK) or a negative PAL_ERR_* code; pal_last_error() gives the text;
 *   - plain pointers and sizes only; arrays are C-contiguous, row-major, float64 unless noted;
 *   - "host" entry points take host pointers and return when the result is in the caller's
 *     buffers; "_dev" entry points take device (HBM) pointers obtained from pal_device_alloc(),
 *     enqueue on the engine's HIP stream and return immediately - pal_synchronize() waits;
 *   - one engine per HIP device; calls on one handle must be serialised by the caller;
 *   - the caller owns every buffer it passes; the engine owns plans and workspaces it allocates;
 *   - all arithmetic is float64/complex128 like the reference's NumPy path.
 */
#ifndef PAL_HIP_H
#define PAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAL_ABI_VERSION 1

#define PAL_OK 0
#define PAL_ERR_INVALID (-1)     /* bad argument (the Python shim raises ValueError)          */
#define PAL_ERR_HIP (-2)         /* HIP runtime / launch failure                              */
#define PAL_ERR_NOMEM (-3)       /* device or host allocation failed                          */
#define PAL_ERR_UNSUPPORTED (-4) /* size outside the engine's range                           */
#define PAL_ERR_INTERNAL (-5)    /* a kernel reported an internal overflow (see last error)   */
#define PAL_ERR_COMM (-6)        /* RCCL failure                                              */
#define PAL_ERR_MATERIAL (-7)    /* pal_image_sources reached a plane whose material is undefined
                                    (utils.py:93-96); *count holds the plane index            */

#define PAL_MAX_PEAKS 256

/* branch bits of the peak-selection fallback chain (utils.py:153-172) */
#define PAL_BR_ALT_THRESHOLD 1
#define PAL_BR_ARGMAX_NO_PEAKS 2
#define PAL_BR_WINDOW_RETRY 4
#define PAL_BR_ARGMAX_WINDOW 8

typedef struct pal_engine* pal_handle;

/* arguments of get_time_delays_phat (utils.py:121-127) that reach the device */
typedef struct pal_phat_params {
  double fs;                   /* sampling rate                                              */
  double threshold_multiplier; /* utils.py:126                                               */
  double max_expected_delay;   /* seconds; NaN = None (utils.py:127,162)                     */
  int32_t threshold_method;    /* 0 = 'median' and any unknown string, 1 = 'adaptive'        */
  int32_t peak_distance;       /* int(fs * 0.001), computed by the caller (utils.py:151)     */
  int32_t num_peaks;           /* 1..PAL_MAX_PEAKS (utils.py:124)                            */
  int32_t reserved;
} pal_phat_params;

/* one row of the TDOA table: everything main.py:204-225 and utils.py:228-250 read off `corr` */
typedef struct pal_pair_record {
  int32_t k_sel;      /* selected array index k; reported lag = k - (n2-1)      */
  int32_t branch;     /* PAL_BR_* bits                                                      */
  int32_t k_argmax;   /* np.argmax(corr)                                                    */
  int32_t n_sel;      /* number of selected peaks (<= num_peaks)                            */
  double cmax;        /* np.max(corr)  (main.py:223)                                        */
  double cmin;        /* np.min(corr)  (utils.py:233)                                       */
  double snr;         /* compute_snr   (utils.py:238-250); +inf when the noise std is 0     */
  double sel_height;  /* corr[k_sel]                                                        */
} pal_pair_record;

/* ---- lifetime ------------------------------------------------------------------------ */
int pal_abi_version(void);
int pal_create(int device, pal_handle* out);
void pal_destroy(pal_handle h);
const char* pal_last_error(pal_handle h); /* h may be NULL: error of the last failed pal_create */
int pal_synchronize(pal_handle h);
/* transforms processed per launch group (workspace = chunk * M * 16 B); 0 restores the default: 128, and for the pair
 * pipeline (two pairs per transform) 240 where one workspace slot stays below 1 GiB, 32 at least */
int pal_set_chunk(pal_handle h, int chunk);
/* Plans (chirps, chirp spectra, prime-factor tables: a few MB per transform length) are built on first use and cached
 * per length, at most 64 of them (PAL_MAX_PLANS, pal_set_max_plans), least recently used out first; pal_clear_plans drops them all now
 * (after draining the engine's streams).  The reference keeps no such state (numpy.fft plans are per call). */
int pal_clear_plans(pal_handle h);
/* Bound of the plan caches (2 .. 4096; 8-16 MB of HBM per plan).  A stream whose frames come in more distinct lengths than the
 * bound, visited cyclically, would rebuild a plan on every visit (least recently used out first is the worst case for a
 * cycle): stream.tdoa_stream raises the bound to the number of lengths of its batch.  pal_plan_stats: plans built and plans
 * evicted since the engine was created (a run that rebuilds plans shows it there). */
int pal_set_max_plans(pal_handle h, int max_plans);
int pal_plan_stats(pal_handle h, int64_t* built, int64_t* evicted);
/* packed transforms (pairs / 2) one launch group of the all-pairs pipeline carries for frames of L samples */
int pal_pair_group_size(pal_handle h, int L, int32_t* transforms);

/* ---- device buffers (so that a host language needs no HIP binding of its own) ---------- */
int pal_device_alloc(pal_handle h, size_t bytes, void** dptr);
int pal_device_free(pal_handle h, void* dptr);
int pal_upload(pal_handle h, void* dptr, const void* host, size_t bytes);
int pal_download(pal_handle h, void* host, const void* dptr, size_t bytes);

/* ---- hot path A: all-pairs GCC-PHAT + peak selection ----------------------------------
 * Replaces the pair loop main.py:202-228 with get_time_delays_phat (utils.py:121-181),
 * phat_correlation (utils.py:108-119), compute_snr / compute_peak_to_peak_ratio
 * (utils.py:228-250) and np.max(corr) (main.py:223) for every i<j of every trial.
 * frames[B][M][L] -> table[B][P], P = M(M-1)/2, pairs in row-major i<j order.
 * corr (optional, may be NULL) receives [B][P][2L-1]. */
int pal_gcc_phat_all_pairs(pal_handle h, const double* frames, int B, int M, int L, const pal_phat_params* prm,
                           pal_pair_record* table, double* corr);
int pal_gcc_phat_all_pairs_dev(pal_handle h, const double* d_frames, int B, int M, int L, const pal_phat_params* prm,
                               pal_pair_record* d_table);
/* Ordering of the _dev forms: everything is enqueued on the engine's streams and the results are complete after
 * pal_synchronize.  With one peak per row (num_peaks = 1) and no corr the column pass finishes the rows itself
 * (csrc/pfa_cols_fin.h); the call then reads ONE integer back at its end (the number of rows that need the stored-row
 * path - a tie, a peak at the lag window's edge: typically 0.1 % - which it resolves before returning), i.e. it blocks
 * the host for the duration of its own device work.  PAL_FIN=0 keeps the call fully asynchronous (stored rows + finish launch). */
/* Non-finite samples: the reference confines a NaN to the pairs of its own microphone.  Here two pairs share one complex
 * transform, so a frame with a NaN or an infinity makes the batched calls (all_pairs, pairs) fail with PAL_ERR_INVALID
 * (reported by the call itself, or by pal_synchronize for the _dev forms) instead of returning rows that differ from the
 * reference's.  The single-pair entry points below have no partner pair and behave like the reference.
 * Amplitude: wherever two real rows share one complex transform (the forward spectra of the batched PHAT calls, xcorr /
 * sync_measure, fractional_delay, simulate_multipath) each row goes in scaled by an exact power of two to [1, 2) and comes
 * out scaled back, so a row's error is relative to its own max |x| and does not depend on its partner's amplitude (zero
 * rows and rows whose maximum is subnormal keep scale 1). */

/* explicit pair list over rows[R][L]: pairs[P][2] row indices -> table[P].  Carries the 1000 shuffled
 * correlations per pair of bootstrap_significance (utils.py:183-216) as one call (rows = sig1 + shuffles of sig2,
 * pairs = (0, k)); only cmax of each record is used there. */
int pal_gcc_phat_pairs(pal_handle h, const double* rows, int R, int L, const int32_t* pairs, int64_t P,
                       const pal_phat_params* prm, pal_pair_record* table);

/* the same with the rows, the pair list (int32 [P][2]) and the table in HBM; asynchronous like every _dev entry point.
 * This is what a rank calls for its contiguous block of the ordered pair list when ONE large frame (256 microphones,
 * 32 640 pairs) is split over the GPUs of a node: every rank holds the frame and recomputes the spectra locally.
 * A row index outside 0..R-1 is reported as PAL_ERR_INVALID by pal_synchronize. */
int pal_gcc_phat_pairs_dev(pal_handle h, const double* d_rows, int R, int L, const int32_t* d_pairs, int64_t P,
                           const pal_phat_params* prm, pal_pair_record* d_table);

/* The batched calls with K = prm->num_peaks (1 .. PAL_MAX_CANDIDATES = 8) selected peaks per pair instead of one: table[..] as above (the
 * records are those of the first peak, n_sel says how many were selected), and
 *   cand_k[..][P][K] int32: the selected array indices in the selection's order (highest peak first), -1 past n_sel;
 *   cand_h[..][P][K] float64 (may be NULL): corr at those indices, +0.0 past n_sel.
 * A row that ends in an argmax fallback has one candidate.  These are the inputs of pal_tdoa_consensus* below.  The 256-wide selection
 * rows of a launch group stay in engine scratch; a small kernel compacts them into the caller's K columns.  Such a call keeps off the
 * one-peak finishing passes (it stores its rows), so it is slower than its one-peak namesake: DESIGN 6f has the figures. */
int pal_gcc_phat_all_pairs_peaks(pal_handle h, const double* frames, int B, int M, int L, const pal_phat_params* prm,
                                 pal_pair_record* table, int32_t* cand_k, double* cand_h);
int pal_gcc_phat_all_pairs_peaks_dev(pal_handle h, const double* d_frames, int B, int M, int L, const pal_phat_params* prm,
                                     pal_pair_record* d_table, int32_t* d_cand_k, double* d_cand_h);
int pal_gcc_phat_pairs_peaks_dev(pal_handle h, const double* d_rows, int R, int L, const int32_t* d_pairs, int64_t P,
                                 const pal_phat_params* prm, pal_pair_record* d_table, int32_t* d_cand_k, double* d_cand_h);

/* ---- bootstrap significance (utils.py:183-216) on the device -------------------------------
 * The reference shuffles sig2 = row j from NumPy's global RNG 1000 times per pair and keeps the (1 - alpha) percentile of
 * max(PHAT(sig1, shuffled sig2)).  Here shuffle s of pair (i, j) is a pure function of (seed, i, j, s, L, mode, block_size):
 * a counter-based generator in exact 64-bit integer arithmetic (pyaudiolocalization_amd/bootstrap.py restates it bit for
 * bit).  It is keyed on the row indices of the pair, so the results are keyed per pair: they do not depend on the order of
 * the pair list, on which other pairs are listed, or on how the shuffles are cut into rounds (pal_set_chunk).  Statistically
 * equivalent to the reference's shuffles, not bitwise equal to them.
 *   permutation: a keyed bijection of [0, L);  block: the blocks of block_size samples in keyed order, the short last block
 *   keeping its length;  circular: np.roll(row, shift) with a keyed shift in [0, L).
 * Invalid mode, block_size < 1, num_bootstrap (S) < 1 or a row index outside 0..R-1: PAL_ERR_INVALID (the _dev form reports a
 * bad row index of its device pair list through pal_synchronize).  Non-finite samples: as the batched calls above. */
#define PAL_BOOT_PERMUTATION 0
#define PAL_BOOT_BLOCK 1
#define PAL_BOOT_CIRCULAR 2
/* shuffles s0 .. s0+S-1 of row d_row[L] under the key (seed, i, j): d_out[S][L] */
int pal_bootstrap_shuffle_dev(pal_handle h, const double* d_row, int L, int32_t i, int32_t j, int32_t mode, int32_t block_size,
                              uint64_t seed, int64_t s0, int32_t S, double* d_out);
/* peaks[P][S] = max PHAT(rows[i], shuffle s of rows[j]) for every listed pair (i, j) */
int pal_bootstrap_peaks(pal_handle h, const double* rows, int R, int L, const int32_t* pairs, int64_t P, int32_t num_bootstrap,
                        int32_t mode, int32_t block_size, uint64_t seed, double* peaks);
int pal_bootstrap_peaks_dev(pal_handle h, const double* d_rows, int R, int L, const int32_t* d_pairs, int64_t P,
                            int32_t num_bootstrap, int32_t mode, int32_t block_size, uint64_t seed, double* d_peaks);

/* ---- position solve (main.py:233-298) on the device -------------------------------------------
 * TDOA tables -> source positions, batched: per frame the reference's time delays (main.py:204-212), weights
 * (utils.py:484-497), box (utils.py:364-382) and residuals (utils.py:384-405); then, instead of scikit-learn's clustered
 * starts and SciPy's trust-region solver, a fixed start list (0: the mean microphone position, 1 .. grid^3: the cell centres
 * of a grid over the box, x slowest, then n_extra caller starts clipped to the box) and one bounded Levenberg-Marquardt
 * iteration per (frame, start) in float64.  The lowest cost among the starts that ended inside a stop rule wins, exact ties
 * to the lowest start index.  pyaudiolocalization_amd/solve.py states the algorithm step by step (the kernels differ from it
 * only in the order of the sums over the pairs); results do not depend on which other frames share the call.
 *   tables[B][P] (P = M(M-1)/2, row-major i<j), lengths[B] (host: samples per frame, td = (k_sel - (L-1)) / fs),
 *   mics[M][3] (host), calib[M] (host, seconds, or NULL), weights[B][P] (host; PAL_SOLVE_W_ARRAY only),
 *   extra_starts[B][n_extra][3] (host, or NULL when n_extra = 0), out[B] (host).
 * pal_solve_positions_dev takes the tables in HBM (e.g. straight from pal_gcc_phat_all_pairs_dev) and, because its result is
 * a host array, returns when the positions are there.  2 <= M <= 256, 0 <= grid <= 16 with at least one start beside the
 * centre (grid >= 1 or n_extra >= 1), fs > 0, c > 0, buffer >= 0, max_iter >= 1 (0 = the default 200): PAL_ERR_INVALID otherwise. */
#define PAL_SOLVE_W_ONES 0   /* w = 1                                                                  */
#define PAL_SOLVE_W_SNR 1    /* w = snr / mean(snr) of the records, as compute_weights (NumPy's mean)  */
#define PAL_SOLVE_W_ARRAY 2  /* w = the caller's weights[B][P]                                          */
#define PAL_SOLVE_CONVERGED 1    /* the winning start ended inside a stop rule                          */
#define PAL_SOLVE_HIT_CAP 2      /* no start did: the record holds the lowest cost reached at max_iter  */
#define PAL_SOLVE_BAD_WEIGHTS 4  /* a weight is not finite (an infinite SNR, utils.py:248-249): frame not solved, position NaN */
#define PAL_SOLVE_ON_FACE 8      /* a coordinate of the position lies on a face of the box              */
typedef struct pal_solve_params {
  double fs;            /* sampling rate                                                      */
  double c;             /* speed of sound                                                     */
  double buffer;        /* dynamic_bounds_extended's buffer (main.py:246 passes 5.0)          */
  int32_t grid;         /* cells per axis of the start grid (4: 65 starts)                    */
  int32_t max_iter;     /* trial points per start; 0 = 200                                    */
  int32_t weight_mode;  /* PAL_SOLVE_W_*                                                      */
  int32_t n_extra;      /* caller starts per frame                                            */
} pal_solve_params;
typedef struct pal_position_record {   /* 96 bytes */
  double position[3];
  double cost;          /* sum(r^2) / 2 at the position                                       */
  double lower[3];      /* the box                                                            */
  double upper[3];
  int32_t start;        /* index of the winning start (-1: none)                              */
  int32_t iterations;   /* trial points it took                                               */
  int32_t converged_starts;
  int32_t status;       /* PAL_SOLVE_* bits                                                   */
} pal_position_record;
int pal_solve_positions_dev(pal_handle h, const pal_pair_record* d_tables, int B, int M, const int32_t* lengths, const double* mics,
                            const double* calib, const double* weights, const double* extra_starts, const pal_solve_params* prm,
                            pal_position_record* out);
int pal_solve_positions(pal_handle h, const pal_pair_record* tables, int B, int M, const int32_t* lengths, const double* mics,
                        const double* calib, const double* weights, const double* extra_starts, const pal_solve_params* prm,
                        pal_position_record* out);
/* The same solve under a robust loss, for tables with outlier pairs: minimise sum_p C^2 rho(r_p^2 / C^2) / 2 (SciPy's convention;
 * `cost` of the record is that sum) with C = f_scale in metres of weighted residual, finite and positive, and rho(z) = z (LINEAR:
 * the two calls above, f_scale ignored), 2 (sqrt(1 + z) - 1), z | 2 sqrt(z) - 1 beyond z = 1, or ln(1 + z).  pair_weights[B][P]
 * (host, or NULL) receives rho'(z_p) at the returned position: 1 for a pair the fit kept, towards 0 for one it discounted.
 * An unknown loss or a bad f_scale is PAL_ERR_INVALID. */
#define PAL_SOLVE_LOSS_LINEAR 0
#define PAL_SOLVE_LOSS_SOFT_L1 1
#define PAL_SOLVE_LOSS_HUBER 2
#define PAL_SOLVE_LOSS_CAUCHY 3
int pal_solve_positions_loss_dev(pal_handle h, const pal_pair_record* d_tables, int B, int M, const int32_t* lengths, const double* mics,
                                 const double* calib, const double* weights, const double* extra_starts, const pal_solve_params* prm,
                                 pal_position_record* out, int32_t loss, double f_scale, double* pair_weights);
int pal_solve_positions_loss(pal_handle h, const pal_pair_record* tables, int B, int M, const int32_t* lengths, const double* mics,
                             const double* calib, const double* weights, const double* extra_starts, const pal_solve_params* prm,
                             pal_position_record* out, int32_t loss, double f_scale, double* pair_weights);

/* ---- loop closure of TDOA tables: votes and weights (no counterpart in the reference) ------------
 * For three microphones x < y < z the lags of a consistent table close: lag_xy + lag_yz - lag_xz = 0 up to rounding, whatever the
 * geometry, the speed of sound or the calibration delays (calib[j] - calib[i] cancels around a triangle).  A pair whose row picked a
 * multipath or noise peak breaks every triangle it belongs to.  Integer arithmetic on k_sel throughout (lag = k_sel - (lengths[b] - 1)):
 * pyaudiolocalization_amd/closure.py states it index by index and the device equals it bit for bit.
 *   tables[B][P] (P = M(M-1)/2, row-major i<j), lengths[B] (host, read before the call returns);
 *   votes[B][P]: per pair (i, j) the number of third microphones k whose triangle with i and j closes within tol samples;
 *   mic_closed[B][M]: closed triangles that contain microphone m (half the sum of the votes of its pairs);
 *   weights[B][P]: PAL_CLOSURE_W_*, ready to be the weights of pal_solve_positions* under PAL_SOLVE_W_ARRAY;
 *   summary[B].  Each of the four outputs may be NULL, not all of them.  Results do not depend on which other frames share the call.
 * 3 <= M <= 256, B >= 1, 0 <= tol <= 2^20, min_votes >= 0 (above M - 2: every weight is 0), 1 <= lengths[b] <= 2^24, a known mode:
 * PAL_ERR_INVALID otherwise, and for a record whose k_sel lies outside 0..2 lengths[b] - 2 (so that a sum of three lags stays far inside
 * int32): the host form reports it itself, the _dev form - asynchronous like every _dev entry point, results complete after
 * pal_synchronize - through pal_synchronize, like the bad row index of a device pair list.
 * What the check cannot see: a constant clock offset of one microphone shifts all its lags consistently and closes every triangle. */
#define PAL_CLOSURE_W_MASK 0   /* weight = votes >= min_votes ? 1 : 0                */
#define PAL_CLOSURE_W_SOFT 1   /* weight = votes >= min_votes ? votes / (M - 2) : 0  */
typedef struct pal_closure_frame {   /* 16 bytes */
  int32_t closed;      /* triangles x<y<z of the frame with |lag_xy + lag_yz - lag_xz| <= tol   */
  int32_t triangles;   /* M (M-1) (M-2) / 6                                                     */
  int32_t kept_pairs;  /* pairs with weight > 0                                                 */
  int32_t worst_mic;   /* argmin of mic_closed, lowest index at ties                            */
} pal_closure_frame;
int pal_tdoa_closure_dev(pal_handle h, const pal_pair_record* d_tables, int B, int M, const int32_t* lengths, int32_t tol,
                         int32_t min_votes, int32_t weight_mode, int32_t* d_votes, int32_t* d_mic_closed, double* d_weights,
                         pal_closure_frame* d_summary);
int pal_tdoa_closure(pal_handle h, const pal_pair_record* tables, int B, int M, const int32_t* lengths, int32_t tol, int32_t min_votes,
                     int32_t weight_mode, int32_t* votes, int32_t* mic_closed, double* weights, pal_closure_frame* summary);

/* ---- loop-closure consensus over several candidate peaks per pair (no counterpart in the reference) ------------
 * The closure check says which pairs are wrong; this call puts them right where the right lag is among the pair's K candidate peaks.
 * Integer arithmetic on array indices throughout (lag = index - (lengths[b] - 1)): pyaudiolocalization_amd/consensus.py states the rule
 * index by index and the device equals it byte for byte.
 *   cand_k[B][P][K]: candidate array indices per pair (P = M(M-1)/2, row-major i<j), highest peak first, -1 = absent; the present
 *     candidates of a pair form a prefix and candidate 0 is present;  cand_h[B][P][K] (may be NULL): their heights;
 *   tables[B][P] (may be NULL when table_out is NULL): the records that table_out copies;  lengths[B] (host, read before the call returns);
 *   stage 0: support of candidate c of pair (i, j) = the third microphones k for which candidates a of pair {i, k} and b of pair {j, k}
 *     exist with |s(i,k,a) - s(j,k,b) - lag(c)| <= tol (s: the lag, negated when the first index is the larger); the first c with the
 *     largest support is taken;  then exactly `rounds` Jacobi rounds: a pair keeps its candidate unless another one has strictly more
 *     closure votes against the lags the other pairs chose in the previous round (then the first c with the most votes);
 *   sel[B][P]: the chosen candidate;  table_out[B][P]: the records with k_sel the chosen candidate, sel_height its height (when cand_h
 *     is given) and PAL_BR_CONSENSUS set where sel != 0;  summary[B].  Each of the three outputs may be NULL, not all of them.
 *     Results do not depend on which other frames share the call.
 * 3 <= M <= 256, 1 <= K <= PAL_MAX_CANDIDATES, B >= 1, 0 <= tol <= 2^20, 0 <= rounds <= PAL_MAX_CONSENSUS_ROUNDS, 1 <= lengths[b] <= 2^24:
 * PAL_ERR_INVALID otherwise, and for a present candidate outside 0..2 lengths[b] - 2, an absent candidate 0 or a gap in the prefix: the
 * host form reports these itself, the _dev form - asynchronous, results complete after pal_synchronize - through pal_synchronize.
 * What the rule cannot see: among two consistent sources (the source and an image source) the rounds converge on the one that the
 * majority of first picks lies on; a constant clock offset of one microphone closes every triangle. */
#define PAL_MAX_CANDIDATES 8
#define PAL_MAX_CONSENSUS_ROUNDS 8
#define PAL_BR_CONSENSUS 16   /* branch bit of table_out: the consensus replaced the first peak */
typedef struct pal_consensus_frame {   /* 16 bytes */
  int32_t moved;          /* pairs with sel != 0                                                   */
  int32_t closed_before;  /* closed triangles (within tol) of the table of candidate 0             */
  int32_t closed_after;   /* ... of the table the call chose                                       */
  int32_t changed_last;   /* pairs that changed in the last round (rounds = 0: in stage 0)         */
} pal_consensus_frame;
int pal_tdoa_consensus_dev(pal_handle h, const pal_pair_record* d_tables, const int32_t* d_cand_k, const double* d_cand_h, int B, int M,
                           int K, const int32_t* lengths, int32_t tol, int32_t rounds, int32_t* d_sel, pal_pair_record* d_table_out,
                           pal_consensus_frame* d_summary);
int pal_tdoa_consensus(pal_handle h, const pal_pair_record* tables, const int32_t* cand_k, const double* cand_h, int B, int M, int K,
                       const int32_t* lengths, int32_t tol, int32_t rounds, int32_t* sel, pal_pair_record* table_out,
                       pal_consensus_frame* summary);

/* ---- steered-response power (SRP-PHAT) map from all-pairs rows (no counterpart in the reference) ---------------
 * For every cell of a grid the map sums, over all pairs, the pair's GCC-PHAT row at the lag the cell's centre predicts: no peak is
 * picked per pair, the table's index mapping plays no part, and several sources show as several maxima.
 * pyaudiolocalization_amd/srp.py states every rule below sample by sample; csrc/srp_math.h is the arithmetic for host and device.
 * Conventions: the row of pair (i, j), i < j, has n = 2L - 1 samples with zero lag at index 0 and peaks at the circular lag d_i - d_j;
 * everything here counts the centred lag s = d_j - d_i in samples (the sign of the closure check): raw[u] = row[(-u) mod n].
 *
 * pal_gcc_phat_all_pairs_strips*: frames[B][M][L] -> strips[B][P][2T+1] (P = M(M-1)/2, row-major i<j) with
 *     strips[..][p][T + s] = sum over u = -W..W of (W + 1 - |u|) * raw_p[s + u]   (increasing u, every product rounded, no fma):
 *   the rows' samples around zero lag, smoothed by a triangle of half-width W (W = 0: the samples themselves).  `table` (may be NULL)
 *   receives the one-peak table of the same rows, as pal_gcc_phat_all_pairs with corr gives it (prm: as there, num_peaks = 1).  The
 *   rows go through engine scratch in slices of whole frames that stay under about 1 GiB where one frame does (one frame of 64
 *   microphones and L = 44 100 alone is 1.4 GB of rows: a slice is never less than one frame).
 *   B >= 1, M >= 2, T >= 0, 0 <= W <= 32, T + W <= L - 1: PAL_ERR_INVALID otherwise.
 *
 * pal_srp_map*: strips[B][P][2T+1] -> power[B][G] over the grid's G = count[0] * count[1] * count[2] cells; cell (ix, iy, iz) has the
 *   linear index g = (ix * count[1] + iy) * count[2] + iz and the centre lo[a] + (i_a + 0.5) * ((hi[a] - lo[a]) / count[a]).
 *     power[g] = sum over p of w_p * strips[p][T + s(g, p)],   s(g, p) = rint(((d_j - d_i) * fs) / c)   (half to even)
 *   with d_m the distance of the centre from microphone m (q = dx*dx; q += dy*dy; q += dz*dz; sqrt(q), every product rounded) and
 *   w_p = pair_weights[b][p], or 1 when pair_weights is NULL.  A term with |s| > T is clipped: it adds nothing and is counted in
 *   summary[b].clipped.  The order of the sum is fixed: the same input gives the same bytes whatever B is.  mics[M][3] and the grid
 *   are host memory, read before the call returns.  With K > 0 the first K peaks of every frame's map go to peaks[B][K] (see
 *   pal_srp_peaks).  power, peaks and summary may each be NULL, not all of them; peaks needs K > 0.
 *   1 <= count[a] <= 1024 (PAL_ERR_INVALID below 1, PAL_ERR_UNSUPPORTED above), G <= 2^24 (PAL_ERR_UNSUPPORTED), hi[a] > lo[a], all
 *   coordinates finite, fs > 0, c > 0, 0 <= K <= PAL_SRP_MAX_PEAKS, 1 <= R <= PAL_SRP_MAX_RADIUS when K > 0, T >= 0, M >= 2, B >= 1.
 *
 * pal_srp_peaks*: power[B][G] -> peaks[B][K].  A cell is a peak iff it is not NaN and no cell of its (2R+1)^3 neighbourhood, cut at
 *   the grid's border, is higher or is equal with a lower linear index.  The peaks are ordered by power descending, then by index;
 *   the first K are written, absent entries as index -1 and all else 0.  summary (may be NULL): n_peaks = entries present, clipped = 0.
 *   1 <= K <= PAL_SRP_MAX_PEAKS, 1 <= R <= PAL_SRP_MAX_RADIUS.
 *
 * pal_srp_zoom*: strips[B][P][2T+1], seeds[B][K] (pal_srp_peak, as pal_srp_map writes them) -> out[B][K]: a coarse-to-fine search
 *   around every seed with a continuous rule (srp.zoom).  A level has a centre and a half-extent per axis; its Z^3 points are the cell
 *   centres of the box centre -+ half-extent, by the map's own point and index arithmetic.  Level 0: the seed's (x, y, z) and half0[3]
 *   (metres).  The power of a point sums, over the pairs in the order of the map kernel's microphone tiles (srp.tile_order),
 *     w_p * (s0 + f * (s1 - s0)),   q = ((d_j - d_i) * fs) / c,  k = floor(q),  f = q - k,  s0 = strips[p][T + k],  s1 = strips[p][T + k + 1]
 *   every product rounded; a term with k < -T or k > T - 1 (or q not finite) is clipped: it adds nothing and is counted.  The best cell
 *   of a level is the first by (power descending, index ascending) among the cells that are not NaN; the next level has its centre and
 *   the half-extent (hi - lo) / Z, one cell.  Where every cell of a level is NaN the zoom stops: the record keeps the centre that level
 *   started from, power = NaN and the levels completed before it.  A seed with index < 0 is absent: seed = -1 and all else 0.  The
 *   order of every sum is fixed: the same input gives the same bytes whatever B and K are, and they are the specification's bytes.
 *   mics[M][3] and half0[3] are host memory, read before the call returns.
 *   2 <= Z <= PAL_SRP_MAX_ZOOM_CELLS, 1 <= levels <= PAL_SRP_MAX_ZOOM_LEVELS, 1 <= K <= PAL_SRP_MAX_PEAKS, T >= 1, every half0[a]
 *   finite and > 0, microphone coordinates finite, fs > 0, c > 0, M >= 2, B >= 1, no NULL buffer but d_pair_weights: PAL_ERR_INVALID
 *   otherwise; M > 4096: PAL_ERR_UNSUPPORTED.
 *
 * pal_srp_doa*: the direction map, for arrays that resolve direction and not range: strips[B][P][2T+1] -> power[B][G] over
 *   G = n_az * n_el directions under the plane-wave model.  The device evaluates no sine: az[n_az][2] = (cos, sin) of every azimuth and
 *   el[n_el][2] = (cos, sin) of every elevation are host tables (srp.doa_axes builds them at the cell centres).  Cell (ia, ie) has the
 *   linear index g = ia * n_el + ie and the direction ux = ce * ca, uy = ce * sa, uz = se; the entries must be finite, not unit vectors.
 *     a_m = ux * mx; a_m += uy * my; a_m += uz * mz   (every product rounded),   s(g, p) = rint(((a_i - a_j) * fs) / c)   for p = (i, j)
 *     power[g] = sum over p of w_p * strips[p][T + s(g, p)]
 *   with the clip rule and the counters of pal_srp_map, the terms added in the order of the map kernel's microphone tiles
 *   (srp.tile_order): the bytes are the specification's (srp.doa_map) on any strips, whatever B is.  With K > 0 the first K peaks of
 *   every frame's map go to peaks[B][K] (see pal_srp_doa_peaks).  power, peaks and summary may each be NULL, not all; peaks needs K > 0.
 *   mics, grid, az and el are host memory in both forms, read before the call returns.
 *   1 <= n_az, n_el <= 1024 (PAL_ERR_INVALID below 1, PAL_ERR_UNSUPPORTED above), table entries and microphone coordinates finite,
 *   fs > 0, c > 0, 0 <= K <= PAL_SRP_MAX_PEAKS, 1 <= R <= PAL_SRP_MAX_RADIUS when K > 0, T >= 0, M >= 2 (M > 4096:
 *   PAL_ERR_UNSUPPORTED), B >= 1.
 *
 * pal_srp_doa_peaks*: power[B][n_az][n_el] -> peaks[B][K].  Cell (ia, ie) is a peak iff it is not NaN and no cell at offsets (da, de)
 *   in -R..R is higher, or equal with a lower linear index; elevation is cut at the border, azimuth is taken mod n_az when
 *   grid->wrap != 0 and cut otherwise.  Order, absent entries and summary as pal_srp_peaks; a record's x, y, z is the cell's direction.
 *
 * pal_srp_doa_zoom*: the zoom on the sphere (srp.doa_zoom), again without trigonometry.  A level has a centre u and one half-extent h
 *   in tangent units (radians for small h); level 0 takes the seed's (x, y, z) as given and half0.  e1 = (k x u) / |k x u| with k the
 *   coordinate axis of the smallest |u_k| (the lowest axis wins ties), e2 = u x e1; the offsets are the cell centres of -h .. h in Z
 *   cells; cell (i, j), index i * Z + j, has the point (u + off_i e1 + off_j e2) / |..|, and its power sums pal_srp_zoom's interpolated
 *   term at q = ((a_i - a_j) * fs) / c in tile order.  Best cell, next level (that point, half-extent 2h / Z), stop rule, absent seeds
 *   and the record are pal_srp_zoom's, the record's x, y, z being the direction.  A seed whose direction is zero or not finite gives
 *   what this arithmetic gives.  2 <= Z <= 16, 1 <= levels <= 16, 1 <= K <= 8, T >= 1, half0 finite and > 0: PAL_ERR_INVALID otherwise.
 *
 * The _dev forms are asynchronous on the engine's stream (results complete after pal_synchronize); every `d_` pointer comes from
 * pal_device_alloc.  Every argument check is made before any buffer is touched. */
#define PAL_SRP_MAX_SMOOTH 32
#define PAL_SRP_MAX_PEAKS 8
#define PAL_SRP_MAX_RADIUS 4
#define PAL_SRP_MAX_ZOOM_CELLS 16
#define PAL_SRP_MAX_ZOOM_LEVELS 16
typedef struct pal_srp_grid {    /* 64 bytes */
  double lo[3], hi[3];    /* the box                                                               */
  int32_t count[3];       /* cells per axis                                                        */
  int32_t reserved;
} pal_srp_grid;
typedef struct pal_srp_peak {    /* 40 bytes */
  double x, y, z;         /* the cell's centre                                                     */
  double power;           /* the map at that cell                                                  */
  int32_t index;          /* its linear index, -1 = absent                                         */
  int32_t reserved;
} pal_srp_peak;
typedef struct pal_srp_frame {   /* 16 bytes */
  int64_t clipped;        /* terms of the map's sums with |s| > T                                  */
  int32_t n_peaks;        /* entries present in the frame's peaks                                  */
  int32_t reserved;
} pal_srp_frame;
typedef struct pal_srp_zoom_record {   /* 48 bytes: one (frame, seed) of pal_srp_zoom (a typedef and a function cannot share a name in C) */
  double x, y, z;         /* the best cell's centre at the last completed level                    */
  double power;           /* the power of that cell; NaN where a level had no cell that is not NaN */
  int64_t clipped;        /* terms clipped over all cells of all levels run                        */
  int32_t seed;           /* the seed record's index, -1 = absent (then all else 0)                */
  int32_t levels;         /* levels completed                                                      */
} pal_srp_zoom_record;
int pal_gcc_phat_all_pairs_strips_dev(pal_handle h, const double* d_frames, int B, int M, int L, const pal_phat_params* prm, int T, int W,
                                      pal_pair_record* d_table, double* d_strips);
int pal_gcc_phat_all_pairs_strips(pal_handle h, const double* frames, int B, int M, int L, const pal_phat_params* prm, int T, int W,
                                  pal_pair_record* table, double* strips);
int pal_srp_map_dev(pal_handle h, const double* d_strips, int B, int M, int T, const double* mics, double fs, double c,
                    const pal_srp_grid* grid, const double* d_pair_weights, int K, int R, double* d_power, pal_srp_peak* d_peaks,
                    pal_srp_frame* d_summary);
int pal_srp_map(pal_handle h, const double* strips, int B, int M, int T, const double* mics, double fs, double c, const pal_srp_grid* grid,
                const double* pair_weights, int K, int R, double* power, pal_srp_peak* peaks, pal_srp_frame* summary);
int pal_srp_peaks_dev(pal_handle h, const double* d_power, int B, const pal_srp_grid* grid, int K, int R, pal_srp_peak* d_peaks,
                      pal_srp_frame* d_summary);
int pal_srp_peaks(pal_handle h, const double* power, int B, const pal_srp_grid* grid, int K, int R, pal_srp_peak* peaks,
                  pal_srp_frame* summary);
int pal_srp_zoom_dev(pal_handle h, const double* d_strips, int B, int M, int T, const double* mics, double fs, double c,
                     const double* d_pair_weights, const pal_srp_peak* d_seeds, int K, const double* half0, int Z, int levels,
                     pal_srp_zoom_record* d_out);
int pal_srp_zoom(pal_handle h, const double* strips, int B, int M, int T, const double* mics, double fs, double c,
                 const double* pair_weights, const pal_srp_peak* seeds, int K, const double* half0, int Z, int levels,
                 pal_srp_zoom_record* out);
typedef struct pal_srp_doa_grid {   /* 16 bytes */
  int32_t n_az, n_el;     /* azimuths and elevations: the lengths of the two tables                */
  int32_t wrap;           /* != 0: the azimuths close the circle, the peak rule takes them mod n_az */
  int32_t reserved;
} pal_srp_doa_grid;
int pal_srp_doa_dev(pal_handle h, const double* d_strips, int B, int M, int T, const double* mics, double fs, double c,
                    const pal_srp_doa_grid* grid, const double* az, const double* el, const double* d_pair_weights, int K, int R,
                    double* d_power, pal_srp_peak* d_peaks, pal_srp_frame* d_summary);
int pal_srp_doa(pal_handle h, const double* strips, int B, int M, int T, const double* mics, double fs, double c,
                const pal_srp_doa_grid* grid, const double* az, const double* el, const double* pair_weights, int K, int R, double* power,
                pal_srp_peak* peaks, pal_srp_frame* summary);
int pal_srp_doa_peaks_dev(pal_handle h, const double* d_power, int B, const pal_srp_doa_grid* grid, const double* az, const double* el,
                          int K, int R, pal_srp_peak* d_peaks, pal_srp_frame* d_summary);
int pal_srp_doa_peaks(pal_handle h, const double* power, int B, const pal_srp_doa_grid* grid, const double* az, const double* el, int K,
                      int R, pal_srp_peak* peaks, pal_srp_frame* summary);
int pal_srp_doa_zoom_dev(pal_handle h, const double* d_strips, int B, int M, int T, const double* mics, double fs, double c,
                         const double* d_pair_weights, const pal_srp_peak* d_seeds, int K, double half0, int Z, int levels,
                         pal_srp_zoom_record* d_out);
int pal_srp_doa_zoom(pal_handle h, const double* strips, int B, int M, int T, const double* mics, double fs, double c,
                     const double* pair_weights, const pal_srp_peak* seeds, int K, double half0, int Z, int levels,
                     pal_srp_zoom_record* out);

/* single-pair signatures: phat_correlation(sig1, sig2) (utils.py:108) -> corr[n1+n2-1] */
int pal_phat_correlation(pal_handle h, const double* sig1, int n1, const double* sig2, int n2, double* corr);
/* get_time_delays_phat (utils.py:121): corr[n1+n2-1] (may be NULL), k_out[num_peaks] array indices */
int pal_get_time_delays_phat(pal_handle h, const double* sig1, int n1, const double* sig2, int n2,
                             const pal_phat_params* prm, int32_t* k_out, pal_pair_record* rec, double* corr);
/* compute_snr / compute_peak_to_peak_ratio / max on an existing correlation row (utils.py:228-250) */
int pal_corr_metrics(pal_handle h, const double* corr, int n, pal_pair_record* rec);
/* get_time_delays_phat's selection (utils.py:144-179) and the record's metrics on existing rows: corr[R][n] (host),
 * n2 as in the lag mapping k - (n2 - 1), table[R], k_out[R][num_peaks] (may be NULL; -1 past n_sel).  A non-finite
 * sample is PAL_ERR_INVALID, found on the host before anything is launched. */
int pal_select_peaks(pal_handle h, const double* corr, int R, int n, int n2, const pal_phat_params* prm,
                     pal_pair_record* table, int32_t* k_out);

/* ---- hot path B: image-source multipath simulation ------------------------------------
 * generate_image_sources_iterative (utils.py:67-106): host C++, discovery order preserved.
 * planes[K][4], material_id[K] index into absorption[]/freq_coeff[] (n_materials entries, -1 = undefined);
 * images[cap][3], image_material[cap]; *count receives the number found (PAL_ERR_UNSUPPORTED if > cap). */
int pal_image_sources(const double* source, const double* planes, const int32_t* material_id, int K,
                      const double* absorption, const double* freq_coeff, int n_materials, int max_order,
                      double frequency, const double* mics, int M, double threshold, int round_decimals,
                      double* images, int32_t* image_material, int cap, int* count);
/* simulate_signals_with_multipath (main.py:103-123) after the path geometry is known:
 * base[B][nbase] zero-padded to total_samples, delays/gains[B][M][K] (seconds, linear gain, fp64),
 * out[B][M][out_len] with out_len = trim_len if 0 < trim_len < total_samples, else total_samples (the slice
 * [:trim_len] of main.py:119-120 never lengthens a row); fractional_delay (signal_processing.py:66-80),
 * normalize_signal + dynamic_range_compression (:82-94) fused.  100 <= total_samples <= 2^19 and nbase <= total_samples,
 * or the call is refused.  A microphone whose gains are all zero gives an all-zero row, as the reference's sum does. */
int pal_simulate_multipath(pal_handle h, const double* base, int B, int nbase, double fs, int total_samples,
                           const double* delays, const double* gains, int M, int K, int trim_len, double* out);
/* fractional_delay(signal, delay, fs) alone (signal_processing.py:66-80); rows[R][N], delay per row */
int pal_fractional_delay(pal_handle h, const double* rows, int R, int N, const double* delays, double fs, double* out);
/* Delay-and-sum beamformer (specification: pyaudiolocalization_amd/beamform.py, steer): frames[B][M][L] steered at S points per frame,
 *   out[b][s] = sum_m weights[b][s][m] * fractional_delay(frames[b][m], delays[b][s][m], fs)      (the sum is formed on the spectra, m ascending,
 *   one inverse transform and one fade window per beam); delays / weights[B][S][M] (seconds, any sign), out[B][S][L].
 * 100 <= L <= 2^19, B, M, S >= 1.  PAL_ERR_INVALID: a NULL pointer, fs not positive and finite, a delay or weight that is not finite,
 * |delay| fs > L, a non-finite sample anywhere in `frames` (rows share transforms: the whole call fails).  A beam whose weighted rows are
 * all silent (all weights zero, or frames of zeros) is a row of exact zeros.  The _dev form is asynchronous and takes every pointer from
 * pal_device_alloc; what it finds in the tables or the samples is reported by pal_synchronize, and d_out is not valid then. */
int pal_steer_sum(pal_handle h, const double* frames, int B, int M, int L, double fs, const double* delays, const double* weights, int S,
                  double* out);
int pal_steer_sum_dev(pal_handle h, const double* d_frames, int B, int M, int L, double fs, const double* d_delays,
                      const double* d_weights, int S, double* d_out);
/* Null-steering beamformer (specification: pyaudiolocalization_amd/beamform.py, separate): the S beams of a frame cancel each other's
 * sources.  Per frequency bin Z = (G + delta I)^-1 Y, with Y the delay-and-sum spectra of pal_steer_sum at weights = gains, G the S x S
 * Gram matrix of the steering vectors gains[b][s][m] exp(j 2 pi f delays[b][s][m]) and delta = loading * max_s sum_m gains[b][s][m]^2;
 * out[b][s] = ifft(Z[s]).real[:L] * fade_window(L).  With S = 1 and loading 0 that is pal_steer_sum at weights gains / sum_m gains^2.
 * Everything pal_steer_sum refuses is refused the same way; also PAL_ERR_INVALID: loading negative or not finite, loading == 0 with
 * S > 1 (bin 0 of G is singular); PAL_ERR_UNSUPPORTED: S > 8.  A source whose gains are all zero is a row of exact zeros beside the
 * others, a frame without a live weighted row is S rows of exact zeros.  The _dev form is asynchronous like pal_steer_sum_dev. */
int pal_separate(pal_handle h, const double* frames, int B, int M, int L, double fs, const double* delays, const double* gains, int S,
                 double loading, double* out);
int pal_separate_dev(pal_handle h, const double* d_frames, int B, int M, int L, double fs, const double* d_delays, const double* d_gains,
                     int S, double loading, double* d_out);
/* MVDR beamformer (specification: pyaudiolocalization_amd/beamform.py, mvdr): weights from the frames' own covariance.  The B frames are
 * G groups of Q = B / G consecutive frames, the snapshots of one covariance under one steering table delays / gains[G][S][M].  Per
 * group and frequency bin R = sum_b X[b] X[b]^H, R~ = R + loading (tr R / M) I, a[m] = gains[g][s][m] exp(j 2 pi f delays[g][s][m]),
 * w = R~^-1 a / (a^H R~^-1 a) by Cholesky, and out[b][s] = ifft(w^H X[b]).real[:L] * fade_window(L), out[B][S][L]: the beam passes
 * what arrives with the delays of source s unchanged and has the least power otherwise, so a stationary interferer nobody located
 * is cancelled.  weights: NULL, or [G][S][M][L + 1] complex values as interleaved doubles (the bins 0 .. L of the 2L-point spectrum;
 * w(-f) = conj(w(f))).  Everything pal_steer_sum refuses is refused the same way (the tables hold G S M entries); also
 * PAL_ERR_INVALID: G < 1, B % G != 0, loading not finite or <= 0; PAL_ERR_UNSUPPORTED: M > 64, or a covariance triangle
 * M (M + 1) / 2 x (L + 1) x 16 bytes above 4 GiB.  A source whose gains are all zero is a row of exact zeros (weights of zero), a
 * frame of zeros in a live group too.  The _dev form is asynchronous like pal_steer_sum_dev; d_weights may be NULL. */
int pal_mvdr(pal_handle h, const double* frames, int B, int M, int L, double fs, const double* delays, const double* gains, int G, int S,
             double loading, double* out, double* weights);
int pal_mvdr_dev(pal_handle h, const double* d_frames, int B, int M, int L, double fs, const double* d_delays, const double* d_gains, int G,
                 int S, double loading, double* d_out, double* d_weights);
/* normalize_signal (normalize_only != 0) or dynamic_range_compression (signal_processing.py:82-94) */
int pal_normalize_compress(pal_handle h, const double* rows, int R, int N, int normalize_only, double threshold,
                           double epsilon, double* out);

/* ---- prefilter and synchronisation ------------------------------------------------------
 * noise_reduction (signal_processing.py:109-138): filtfilt(b, a, x) with scipy's defaults (odd
 * extension 3*max(nb,na), lfilter_zi initial state `zi`, designed on the host); rows[R][N]. */
int pal_filtfilt(pal_handle h, const double* b, int nb, const double* a, int na, const double* zi,
                 const double* rows, int R, int N, double* out);
int pal_wiener3(pal_handle h, const double* rows, int R, int N, double* out);
/* synchronize_signals_improved (utils.py:415-427): full cross-correlation of every row against row
 * ref_idx; kpk = argmax|corr| (index into the 2N-1 sequence), win5 = corr[kpk-2..kpk+2] (NaN outside),
 * pkabs = |corr[kpk]|, *refpk = max|autocorrelation of the reference|. */
int pal_xcorr_vs_ref(pal_handle h, const double* rows, int R, int N, int ref_idx, int32_t* kpk, double* win5,
                     double* pkabs, double* refpk);

/* ---- device-resident stage chain (main.py:165-204 without host copies of the waveforms) ----------------------------
 * The streaming configuration (64 microphones x 1024 frames, multipath simulation on) keeps every waveform in HBM:
 * simulate -> measure the synchronisation shifts -> align -> prefilter -> all pairs.  The host supplies the path tables
 * and the filter coefficients and reads back five numbers per row (the 5-point spline refinement and the integer pads of
 * utils.py:428-451 stay host work, as in pal_xcorr_vs_ref).  All `d_` pointers come from pal_device_alloc.
 *
 * pal_simulate_multipath_dev: as pal_simulate_multipath with d_base[B][nbase], d_delays / d_gains[B][M][K], d_out[B][M][out_len].
 * pal_row_energies_dev: energy[r] = sum of squares of row r of d_rows[R][N] (device summation order: last-bit differences
 *   from numpy's np.sum(sig**2) - the caller settles near-ties of utils.py:413-414 with numpy itself, engine.sync_measure_dev).
 * pal_sync_measure_dev: per frame b of d_rows[B][M][N]: ref_idx[b] (IN / OUT: >= 0 on entry = use this reference microphone;
 *   < 0 = argmax of the device's row energies, utils.py:413-414), then
 *   pal_xcorr_vs_ref of the frame's rows against that row: kpk[B][M], win5[B][M][5], pkabs[B][M], refpk[B] (host arrays).
 * pal_align_rows_dev: utils.py:448-456 - d_out[r][pad_left[r] + i] = d_rows[r][i], zeros elsewhere (rows of Lout samples).
 * pal_filtfilt_dev / pal_wiener3_dev: as pal_filtfilt / pal_wiener3 on rows in HBM (b, a, zi stay host arrays). */
int pal_simulate_multipath_dev(pal_handle h, const double* d_base, int B, int nbase, double fs, int total_samples,
                               const double* d_delays, const double* d_gains, int M, int K, int trim_len, double* d_out);
int pal_row_energies_dev(pal_handle h, const double* d_rows, int R, int N, double* energy);
int pal_sync_measure_dev(pal_handle h, const double* d_rows, int B, int M, int N, int32_t* ref_idx, int32_t* kpk,
                         double* win5, double* pkabs, double* refpk);
int pal_align_rows_dev(pal_handle h, const double* d_rows, int R, int N, const int32_t* pad_left, int Lout, double* d_out);
int pal_filtfilt_dev(pal_handle h, const double* b, int nb, const double* a, int na, const double* zi, const double* d_rows,
                     int R, int N, double* d_out);
int pal_wiener3_dev(pal_handle h, const double* d_rows, int R, int N, double* d_out);
/* the same filter over R rows of DIFFERENT lengths in one launch (the frames of a stream have their own synchronised
 * lengths, utils.py:448-456): row r is d_in[in_off[r] .. + lengths[r]) -> d_out[out_off[r] .. + lengths[r]) (host arrays
 * of offsets in doubles and lengths).  One lane per row, 64 rows per wavefront: a launch takes the same time for 64 rows
 * as for 65 536, so the caller batches. */
int pal_filtfilt_ragged_dev(pal_handle h, const double* b, int nb, const double* a, int na, const double* zi, const double* d_in,
                            double* d_out, int R, const int64_t* in_off, const int64_t* out_off, const int32_t* lengths);

/* ---- recorded audio: resample, normalise, cut frames (utils.py:459-482 in front of the stage chain above) ---------------
 * pal_resample: signal_processing.resample_kaiser_best along the rows of rows[R][N] -> out[R][n_out], n_out = (int)(N * ratio),
 *   ratio = target_fs / original_fs, bit for bit the host function's result (one lane per output sample, the filter taps in
 *   the host function's order, every product rounded before it is added).  n_out_capacity: samples per row that `out` holds;
 *   *n_out is set whenever the rates and N are valid, also when the capacity is too small (PAL_ERR_INVALID) and when `out` is
 *   NULL (a length query: nothing runs).  A rate that is not positive or n_out < 1: PAL_ERR_INVALID.  Ratios whose output
 *   would reach 2^31 samples per row: PAL_ERR_UNSUPPORTED.  pal_resample_dev: rows and out in HBM, asynchronous.
 * pal_resample_set_filter: the right wing of the interpolation filter (win[nwin], num_table entries per zero crossing) as
 *   the host function builds it (_kaiser_best_filter: SciPy's Kaiser window x NumPy's sinc - the engine takes the table
 *   instead of restating those two, so that both sides hold the same bits).  Once per engine, before the first resample;
 *   the engine derives the scaled (win, delta) table of a ratio from it and keeps the latest one in HBM.
 * pal_normalize_compress_dev: pal_normalize_compress on d_rows[R][N] -> d_out[R][N] in HBM (d_out may be d_rows).
 * pal_frame_rows_dev: d_out[f][m][i] = d_rows[m][(first_frame + f) * hop + i] for f < F, m < M, i < frame_len (d_rows[M][T]);
 *   PAL_ERR_INVALID when the last frame would read past T. */
int pal_resample_set_filter(pal_handle h, const double* win, int nwin, int num_table);
int pal_resample(pal_handle h, const double* rows, int R, int N, double original_fs, double target_fs, double* out, int n_out_capacity,
                 int* n_out);
int pal_resample_dev(pal_handle h, const double* d_rows, int R, int N, double original_fs, double target_fs, double* d_out,
                     int n_out_capacity, int* n_out);
int pal_normalize_compress_dev(pal_handle h, const double* d_rows, int R, int N, int normalize_only, double threshold, double epsilon,
                               double* d_out);
int pal_frame_rows_dev(pal_handle h, const double* d_rows, int M, int T, int frame_len, int hop, int first_frame, int F, double* d_out);

/* ---- multi-GPU: one gather of the TDOA table over RCCL/xGMI ------------------------------ */
int pal_comm_unique_id(void* id128);                       /* rank 0; 128-byte ncclUniqueId          */
int pal_comm_init(pal_handle h, int nranks, int rank, const void* id128);
int pal_comm_all_gather(pal_handle h, const void* d_send, void* d_recv, size_t bytes_per_rank);
int pal_comm_destroy(pal_handle h);

/* ---- measurement ---------------------------------------------------------------------------
 * HIP-event timing of the engine's own kernels on its own stream.  Between pal_profile_begin and
 * pal_profile_end every launch is bracketed by events; pal_profile_get returns the summed
 * duration (ms) and launch count of the kernel class `name`, spelled like the kernel's template
 * instance ("k_rows<10,conv>", "k_pfa_rows<11>", "k_peak_stream", ...).  The events cost a few microseconds of
 * idle stream each: pal_profile_sampling(h, every) brackets only every `every`-th launch group of the pair
 * pipeline (averages are unchanged, the run is barely perturbed); the default is 1 = every group. */
int pal_profile_begin(pal_handle h);
int pal_profile_end(pal_handle h);
int pal_profile_sampling(pal_handle h, int every);
int pal_profile_get(pal_handle h, const char* name, double* total_ms, int64_t* launches);
/* enumerate the kernel classes seen so far: index 0.. until PAL_ERR_INVALID */
int pal_profile_entry(pal_handle h, int index, char* name, int cap, double* total_ms, int64_t* launches);
/* transform geometry of the all-pairs plan for frames of L samples: n = 2L-1, conv length M, M1, M2 */
int pal_plan_info(pal_handle h, int L, int32_t* n, int32_t* conv_len, int32_t* m1, int32_t* m2);

/* Prime-factor route of the inverse transform for frame length L: n = n1 * n2 (coprime, odd) with the n2-point
 * DFTs as in-LDS convolutions of `tile_len` points: a chirp convolution (tile_len a power of two >= 2 n2 - 1) or,
 * for n2 = 991, Rader's cyclic convolution (tile_len = n2 - 1 = 990).  All three are 0 when n has no such split
 * (or PAL_PFA=0) and the four-step chirp convolution reported by pal_plan_info does the inverse too. */
int pal_plan_factors(pal_handle h, int L, int32_t* n1, int32_t* n2, int32_t* tile_len);

#ifdef __cplusplus
}
#endif
#endif /* PAL_HIP_H */
