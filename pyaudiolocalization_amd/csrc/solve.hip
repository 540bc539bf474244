// solve.hip - TDOA tables -> source positions on the device (main.py:233-298; pal_solve_positions*).
//
// pyaudiolocalization_amd/solve.py is the specification and solve_math.h its arithmetic.  Three launches per call:
//   k_solve_prepare  one workgroup per frame: time delays, weights (NumPy's pairwise mean for the SNR mode), b = c td w, the
//                    75th percentile of c |td| by an exact radix select, the box and the start list;
//   k_solve_lm       one workgroup per (frame, start): the bounded Levenberg-Marquardt iteration.  Per trial point the lanes
//                    stride over the pairs with sixteen fp64 partial sums each, reduced by the DPP butterflies of wave_reduce.h and
//                    one LDS hop over the wavefronts in a fixed order; every lane then runs the 3 x 3 solve and the bookkeeping
//                    on the same values, so the workgroup needs no broadcast and a result never depends on the batch;
//   k_solve_pick     one wavefront per frame: the winner among the starts.
// A robust loss (pal_solve_positions_loss*; solve.lm_solve_loss) runs k_solve_lm's instantiation for that loss - nineteen sums,
// the pairs reweighted by rho'(z) and rho'(z) + 2 z rho''(z) - and, when the caller asks which pairs the fit discounted,
//   k_solve_weights  one workgroup per frame: rho'(z_p) of every pair at the winning position.
// No floating-point atomics, no waits between workgroups.
#include <algorithm>
#include <cmath>
#include <vector>

#include "engine.h"
#include "solve_math.h"
#include "wave_reduce.h"

namespace pal {

namespace sv = solve;

struct SolveStart {          // result of one (frame, start)
  double x[3];
  double cost;
  int32_t iters, stop;
};
struct SolveFrame {          // per frame, written by k_solve_prepare
  double lo[3], hi[3];
  int32_t status, pad;
};

struct SolveArgs {
  const pal_pair_record* tables;   // [B][P]
  const int32_t* lengths;          // [B]
  const double* mics;              // [M][3]
  const double* calib;             // [M] or nullptr
  const double* weights;           // [B][P] or nullptr
  const double* extra;             // [B][n_extra][3] or nullptr
  const int32_t* pair_idx;         // [P]: i | j << 16
  double2* bw;                     // [B][P]: (b, w)
  double* v;                       // [B][P]: c |td|
  double* starts;                  // [B][S][3]
  SolveFrame* frames;              // [B]
  SolveStart* results;             // [B][S]
  pal_position_record* out;        // [B]
  double* pair_weights;            // [B][P] or nullptr (robust losses only)
  int B, M, P, S;
  int grid, n_extra, max_iter, weight_mode;
  double fs, c, buffer;
  double c2, inv_c2;               // f_scale^2 and its reciprocal (robust losses only)
  int loss;
};

constexpr int kPrepThreads = 256;

__global__ __launch_bounds__(kPrepThreads) void k_solve_prepare(SolveArgs a) {
  __shared__ int hist[256];
  __shared__ int32_t leaf_off[sv::kNpMaxLeaves], leaf_len[sv::kNpMaxLeaves], program[sv::kNpMaxProgram];
  __shared__ double leaf_sum[sv::kNpMaxLeaves];
  __shared__ int sh_i[4];                     // leaves, program length, not-finite flag, count <= value
  __shared__ unsigned long long sh_u[3];      // radix prefix, remaining rank, smallest value above
  __shared__ double sh_mean;
  const int b = blockIdx.x, tid = threadIdx.x, P = a.P;
  const pal_pair_record* tab = a.tables + size_t(b) * P;
  double2* bw = a.bw + size_t(b) * P;
  double* v = a.v + size_t(b) * P;
  const double lm1 = double(a.lengths[b] - 1);
  if (tid == 0) { sh_i[0] = sh_i[1] = sh_i[2] = sh_i[3] = 0; sh_mean = 1.0; }
  __syncthreads();
  // ---- the SNR mean, summed like np.mean
  if (a.weight_mode == PAL_SOLVE_W_SNR) {
    if (tid == 0) {
      int np = 0;
      sh_i[0] = sv::np_plan(P, leaf_off, leaf_len, program, &np);
      sh_i[1] = np;
    }
    __syncthreads();
    auto snr = [&](int64_t p) { return tab[p].snr; };
    for (int l = tid; l < sh_i[0]; l += kPrepThreads) leaf_sum[l] = sv::np_leaf_sum(snr, leaf_off[l], leaf_len[l]);
    __syncthreads();
    if (tid == 0) sh_mean = sv::np_run_program(program, sh_i[1], leaf_sum) / double(P);
    __syncthreads();
  }
  const double mean = sh_mean;
  // ---- time delays, weights, b
  bool finite = true;
  for (int p = tid; p < P; p += kPrepThreads) {
    double td = (double(tab[p].k_sel) - lm1) / a.fs;
    if (a.calib) {
      const int ij = a.pair_idx[p];
      td = td - (a.calib[ij >> 16] - a.calib[ij & 0xffff]);
    }
    double w = 1.0;
    if (a.weight_mode == PAL_SOLVE_W_SNR) w = mean != 0 ? tab[p].snr / mean : tab[p].snr;
    else if (a.weight_mode == PAL_SOLVE_W_ARRAY) w = a.weights[size_t(b) * P + p];
    finite = finite && isfinite(w);
    const double ctd = a.c * td;
    bw[p] = make_double2(ctd * w, w);
    v[p] = fabs(ctd);
  }
  if (!finite) atomicOr(&sh_i[2], 1);
  // ---- rank `lo` of v by a radix select over the bit patterns (non-negative doubles order like their bits), most significant byte first
  double t = 0.0;
  const unsigned long long rank = (unsigned long long)sv::percentile75_rank(P, &t);
  if (tid == 0) { sh_u[0] = 0; sh_u[1] = rank; sh_u[2] = ~0ull; }
  for (int d = 7; d >= 0; --d) {
    hist[tid] = 0;                            // kPrepThreads == 256 bins
    __syncthreads();
    const unsigned long long prefix = sh_u[0];
    for (int p = tid; p < P; p += kPrepThreads) {   // every thread reads back the elements it wrote itself
      const unsigned long long bits = (unsigned long long)__double_as_longlong(v[p]);
      if (d == 7 || (bits >> (8 * (d + 1))) == prefix) atomicAdd(&hist[int((bits >> (8 * d)) & 255)], 1);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned long long k = sh_u[1];
      int bin = 0;
      while (bin < 255 && k >= (unsigned long long)hist[bin]) { k -= (unsigned long long)hist[bin]; ++bin; }
      sh_u[0] = (prefix << 8) | (unsigned long long)bin;
      sh_u[1] = k;
    }
    __syncthreads();
  }
  const unsigned long long vbits = sh_u[0];
  int le = 0;
  unsigned long long above = ~0ull;
  for (int p = tid; p < P; p += kPrepThreads) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v[p]);
    if (bits <= vbits) ++le;
    else if (bits < above) above = bits;
  }
  atomicAdd(&sh_i[3], le);
  atomicMin(&sh_u[2], above);
  __syncthreads();
  const double a_lo = __longlong_as_double((long long)vbits);
  const double a_hi = ((unsigned long long)sh_i[3] >= rank + 2 || sh_u[2] == ~0ull) ? a_lo : __longlong_as_double((long long)sh_u[2]);
  const double pct = sv::percentile_lerp(a_lo, a_hi, t);
  // ---- box and starts (every thread computes the box: M <= 256 microphones)
  double mn[3], mx[3], sum[3] = {0, 0, 0}, lo[3], hi[3];
  for (int k = 0; k < 3; ++k) { mn[k] = a.mics[k]; mx[k] = a.mics[k]; }
  for (int m = 0; m < a.M; ++m)
    for (int k = 0; k < 3; ++k) {
      const double q = a.mics[3 * m + k];
      mn[k] = fmin(mn[k], q);
      mx[k] = fmax(mx[k], q);
      sum[k] = sum[k] + q;
    }
  sv::box_from(mn, mx, pct, a.buffer, lo, hi);
  if (tid == 0) {
    SolveFrame f;
    for (int k = 0; k < 3; ++k) { f.lo[k] = lo[k]; f.hi[k] = hi[k]; }
    f.status = sh_i[2] ? PAL_SOLVE_BAD_WEIGHTS : 0;
    f.pad = 0;
    a.frames[b] = f;
  }
  const int cells = a.grid * a.grid * a.grid;
  for (int s = tid; s < a.S; s += kPrepThreads) {
    double x[3];
    if (s == 0) {
      for (int k = 0; k < 3; ++k) x[k] = sum[k] / double(a.M);
    } else if (s <= cells) {
      sv::grid_start(s - 1, a.grid, lo, hi, x);
    } else {
      const double* e = a.extra + (size_t(b) * a.n_extra + size_t(s - 1 - cells)) * 3;
      for (int k = 0; k < 3; ++k) x[k] = sv::clip(e[k], lo[k], hi[k]);
    }
    double* dst = a.starts + (size_t(b) * a.S + s) * 3;
    dst[0] = x[0]; dst[1] = x[1]; dst[2] = x[2];
  }
}

// One workgroup of T lanes per (frame, start).  LDS: the microphones (6 KB at M = 256), their ten terms at the trial point
// (20 KB), the wavefronts' partial sums.  LOSS: sv::kLossLinear is the sum of squares on sixteen sums; a robust loss carries nineteen.
template <int T, int LOSS = sv::kLossLinear>
__global__ __launch_bounds__(T) void k_solve_lm(SolveArgs a) {
  constexpr int W = T / 64;
  constexpr int NS = LOSS == sv::kLossLinear ? sv::kSums : sv::kSumsLoss;
  __shared__ double mic[sv::kMaxMics * 3];
  __shared__ double terms[sv::kMaxMics * sv::kMicTerms];
  __shared__ double red[W * NS];
  const int b = blockIdx.x / a.S, s = blockIdx.x % a.S, tid = threadIdx.x, P = a.P, M = a.M;
  SolveStart* res = a.results + size_t(b) * a.S + s;
  const SolveFrame fr = a.frames[b];
  if (fr.status & PAL_SOLVE_BAD_WEIGHTS) {            // uniform over the workgroup
    if (tid == 0) {
      SolveStart r;
      r.x[0] = r.x[1] = r.x[2] = r.cost = __builtin_nan("");
      r.iters = 0;
      r.stop = sv::kStopNone;
      *res = r;
    }
    return;
  }
  for (int k = tid; k < 3 * M; k += T) mic[k] = a.mics[k];
  const double2* bw = a.bw + size_t(b) * P;
  const int32_t* idx = a.pair_idx;
  auto eval = [&](const double* x, double* out) {
    __syncthreads();                                   // the previous point's readers are done (first call: mic[] is written)
    for (int m = tid; m < M; m += T) sv::mic_terms(x, mic + 3 * m, terms + sv::kMicTerms * m);
    __syncthreads();
    double acc[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) acc[q] = 0.0;
    for (int p = tid; p < P; p += T) {
      const double2 v = bw[p];
      const int ij = idx[p];
      const double *ti = terms + sv::kMicTerms * (ij & 0xffff), *tj = terms + sv::kMicTerms * (ij >> 16);
      if constexpr (LOSS == sv::kLossLinear) sv::pair_accumulate(acc, ti, tj, v.x, v.y);
      else sv::pair_accumulate_loss<LOSS>(acc, ti, tj, v.x, v.y, a.inv_c2);
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      const double r = wave_sum63(acc[q]);
      if ((tid & 63) == 63) red[(tid >> 6) * NS + q] = r;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      double r = red[q];
#pragma unroll
      for (int w = 1; w < W; ++w) r += red[w * NS + q];
      out[q] = r;
    }
    if constexpr (LOSS != sv::kLossLinear) out[15] = a.c2 * out[15];      // C^2 sum rho(z) in place of rtr
  };
  const double* x0 = a.starts + (size_t(b) * a.S + s) * 3;
  const double start[3] = {x0[0], x0[1], x0[2]};
  SolveStart r;
  sv::lm_solve<NS>(start, fr.lo, fr.hi, a.max_iter, eval, r.x, &r.cost, &r.iters, &r.stop);
  if (tid == 0) *res = r;
}

// The winner of a frame: lowest cost among the starts that ended inside a stop rule, ties to the lowest start index; when none did,
// the lowest cost among the capped ones (PAL_SOLVE_HIT_CAP).
__global__ __launch_bounds__(64) void k_solve_pick(SolveArgs a) {
  __shared__ double bc[2][64];
  __shared__ int bi[2][64], cnt[64];
  const int b = blockIdx.x, lane = threadIdx.x;
  const SolveStart* res = a.results + size_t(b) * a.S;
  double cost[2] = {0, 0};
  int best[2] = {-1, -1}, conv = 0;
  for (int s = lane; s < a.S; s += 64) {              // ascending s per lane: a strict < keeps the lowest index
    const int stop = res[s].stop;
    if (stop == sv::kStopNone) continue;
    const int g = stop == sv::kStopCap ? 1 : 0;
    conv += g == 0;
    const double c = res[s].cost;
    if (best[g] < 0 || c < cost[g]) { best[g] = s; cost[g] = c; }
  }
  for (int g = 0; g < 2; ++g) { bc[g][lane] = cost[g]; bi[g][lane] = best[g]; }
  cnt[lane] = conv;
  __syncthreads();
  if (lane != 0) return;
  const SolveFrame fr = a.frames[b];
  pal_position_record o;
  int total = 0;
  for (int g = 0; g < 2; ++g) {
    best[g] = -1;
    for (int l = 0; l < 64; ++l) {
      if (bi[g][l] < 0) continue;
      if (best[g] < 0 || bc[g][l] < cost[g] || (bc[g][l] == cost[g] && bi[g][l] < best[g])) { best[g] = bi[g][l]; cost[g] = bc[g][l]; }
    }
  }
  for (int l = 0; l < 64; ++l) total += cnt[l];
  for (int k = 0; k < 3; ++k) { o.lower[k] = fr.lo[k]; o.upper[k] = fr.hi[k]; }
  const int win = best[0] >= 0 ? best[0] : best[1];
  o.converged_starts = total;
  o.start = win;
  if (win < 0) {
    o.position[0] = o.position[1] = o.position[2] = o.cost = __builtin_nan("");
    o.iterations = 0;
    o.status = fr.status;
  } else {
    const SolveStart r = res[win];
    int st = best[0] >= 0 ? PAL_SOLVE_CONVERGED : PAL_SOLVE_HIT_CAP;
    for (int k = 0; k < 3; ++k) {
      o.position[k] = r.x[k];
      if (r.x[k] <= fr.lo[k] || r.x[k] >= fr.hi[k]) st |= PAL_SOLVE_ON_FACE;
    }
    o.cost = r.cost;
    o.iterations = r.iters;
    o.status = st | fr.status;
  }
  a.out[b] = o;
}

// rho'(z_p) of every pair at the frame's winning position (NaN where the frame has none): one workgroup per frame, the
// microphones' distances in LDS.
constexpr int kWeightThreads = 256;
__global__ __launch_bounds__(kWeightThreads) void k_solve_weights(SolveArgs a) {
  __shared__ double dist[sv::kMaxMics];
  const int b = blockIdx.x, tid = threadIdx.x, P = a.P;
  const double* x = a.out[b].position;
  for (int m = tid; m < a.M; m += kWeightThreads) {
    const double dx = x[0] - a.mics[3 * m], dy = x[1] - a.mics[3 * m + 1], dz = x[2] - a.mics[3 * m + 2];
    dist[m] = sqrt(dx * dx + dy * dy + dz * dz);
  }
  __syncthreads();
  const double2* bw = a.bw + size_t(b) * P;
  double* dst = a.pair_weights + size_t(b) * P;
  for (int p = tid; p < P; p += kWeightThreads) {
    const double2 v = bw[p];
    const int ij = a.pair_idx[p];
    const double r = (dist[ij >> 16] - dist[ij & 0xffff]) * v.y - v.x;
    dst[p] = sv::loss_d1_of(a.loss, (r * r) * a.inv_c2);
  }
}

int Engine::solve_positions_dev(const pal_pair_record* d_tables, int B, int M, const int32_t* lengths, const double* mics, const double* calib,
                                const double* weights, const double* extra_starts, const pal_solve_params* prm, pal_position_record* out) {
  return solve_positions_impl(d_tables, B, M, lengths, mics, calib, weights, extra_starts, prm, out, sv::kLossLinear, 1.0, nullptr);
}

int Engine::solve_positions_loss_dev(const pal_pair_record* d_tables, int B, int M, const int32_t* lengths, const double* mics, const double* calib,
                                     const double* weights, const double* extra_starts, const pal_solve_params* prm, pal_position_record* out,
                                     int loss, double f_scale, double* pair_weights) {
  if (loss < PAL_SOLVE_LOSS_LINEAR || loss > PAL_SOLVE_LOSS_CAUCHY) return fail(PAL_ERR_INVALID, "unknown loss %d", loss);
  if (!(std::isfinite(f_scale) && f_scale > 0)) return fail(PAL_ERR_INVALID, "f_scale must be finite and positive");
  if (loss != PAL_SOLVE_LOSS_LINEAR)
    return solve_positions_impl(d_tables, B, M, lengths, mics, calib, weights, extra_starts, prm, out, loss, f_scale, pair_weights);
  const int rc = solve_positions_dev(d_tables, B, M, lengths, mics, calib, weights, extra_starts, prm, out);
  if (rc == PAL_OK && pair_weights) std::fill(pair_weights, pair_weights + size_t(B) * (size_t(M) * size_t(M - 1) / 2), 1.0);
  return rc;
}

// loss = sv::kLossLinear takes the sum-of-squares kernels and ignores f_scale and pair_weights
int Engine::solve_positions_impl(const pal_pair_record* d_tables, int B, int M, const int32_t* lengths, const double* mics, const double* calib,
                                 const double* weights, const double* extra_starts, const pal_solve_params* prm, pal_position_record* out,
                                 int loss, double f_scale, double* pair_weights) {
  if (!d_tables || !lengths || !mics || !prm || !out) return fail(PAL_ERR_INVALID, "NULL buffer");
  if (B < 1) return fail(PAL_ERR_INVALID, "need B >= 1");
  if (M < 2) return fail(PAL_ERR_INVALID, "need at least 2 microphones (got %d)", M);
  if (M > sv::kMaxMics) return fail(PAL_ERR_UNSUPPORTED, "%d microphones: the solve holds at most %d", M, sv::kMaxMics);
  if (!(prm->fs > 0)) return fail(PAL_ERR_INVALID, "fs must be positive");
  if (!(prm->c > 0)) return fail(PAL_ERR_INVALID, "the speed of sound must be positive");
  if (!(prm->buffer >= 0)) return fail(PAL_ERR_INVALID, "buffer must not be negative");
  if (prm->grid < 0 || prm->grid > sv::kMaxGrid) return fail(PAL_ERR_INVALID, "grid %d outside 0..%d", prm->grid, sv::kMaxGrid);
  if (prm->n_extra < 0 || prm->n_extra > 4096 || (prm->n_extra > 0 && !extra_starts)) return fail(PAL_ERR_INVALID, "bad extra starts");
  if (prm->grid == 0 && prm->n_extra == 0) return fail(PAL_ERR_INVALID, "no start points: grid = 0 and no extra starts");
  if (prm->max_iter < 0) return fail(PAL_ERR_INVALID, "max_iter must not be negative");
  if (prm->weight_mode < PAL_SOLVE_W_ONES || prm->weight_mode > PAL_SOLVE_W_ARRAY) return fail(PAL_ERR_INVALID, "unknown weight mode %d", prm->weight_mode);
  if (prm->weight_mode == PAL_SOLVE_W_ARRAY && !weights) return fail(PAL_ERR_INVALID, "weight mode 'array' needs weights");
  for (int b = 0; b < B; ++b)
    if (lengths[b] < 1) return fail(PAL_ERR_INVALID, "frame %d: length %d", b, lengths[b]);
  const int P = M * (M - 1) / 2;
  const int S = 1 + prm->grid * prm->grid * prm->grid + prm->n_extra;
  if (int64_t(B) * S > INT32_MAX / 2) return fail(PAL_ERR_UNSUPPORTED, "%d frames x %d starts is too many for one call", B, S);
  // pair -> (i, j), cached per M like the pair table of the all-pairs call
  if (solve_idx_M != M || !solve_idx) {
    std::vector<int32_t> idx;
    idx.reserve(size_t(P));
    for (int i = 0; i < M; ++i)
      for (int j = i + 1; j < M; ++j) idx.push_back(int32_t(i | (j << 16)));
    PAL_HIP(hipStreamSynchronize(stream));
    if (solve_idx) { (void)hipFree(solve_idx); solve_idx = nullptr; }
    PAL_HIP(hipMalloc(&solve_idx, size_t(P) * sizeof(int32_t)));
    PAL_HIP(hipMemcpyAsync(solve_idx, idx.data(), size_t(P) * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    PAL_HIP(hipStreamSynchronize(stream));
    solve_idx_M = M;
  }
  const bool want_pw = loss != sv::kLossLinear && pair_weights;
  // one scratch block: [lengths | mics | calib | weights | extra | bw | v | starts | frames | results | out | pair weights]
  const size_t np = size_t(B) * size_t(P);
  Carve cv;
  const size_t o_len = cv.take(size_t(B) * sizeof(int32_t)), o_mic = cv.take(size_t(M) * 3 * sizeof(double));
  const size_t o_cal = cv.take(calib ? size_t(M) * sizeof(double) : 0);
  const size_t o_wt = cv.take(prm->weight_mode == PAL_SOLVE_W_ARRAY ? np * sizeof(double) : 0);
  const size_t o_ex = cv.take(size_t(B) * size_t(prm->n_extra) * 3 * sizeof(double));
  const size_t o_bw = cv.take(np * sizeof(double2)), o_v = cv.take(np * sizeof(double));
  const size_t o_st = cv.take(size_t(B) * S * 3 * sizeof(double)), o_fr = cv.take(size_t(B) * sizeof(SolveFrame));
  const size_t o_res = cv.take(size_t(B) * S * sizeof(SolveStart)), o_out = cv.take(size_t(B) * sizeof(pal_position_record));
  const size_t o_pw = cv.take(want_pw ? np * sizeof(double) : 0);
  char* base = nullptr;
  PAL_TRY(scratch(kWsSolve, cv.off, &base));
  PAL_HIP(hipMemcpyAsync(base + o_len, lengths, size_t(B) * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  PAL_HIP(hipMemcpyAsync(base + o_mic, mics, size_t(M) * 3 * sizeof(double), hipMemcpyHostToDevice, stream));
  if (calib) PAL_HIP(hipMemcpyAsync(base + o_cal, calib, size_t(M) * sizeof(double), hipMemcpyHostToDevice, stream));
  if (prm->weight_mode == PAL_SOLVE_W_ARRAY) PAL_HIP(hipMemcpyAsync(base + o_wt, weights, np * sizeof(double), hipMemcpyHostToDevice, stream));
  if (prm->n_extra > 0)
    PAL_HIP(hipMemcpyAsync(base + o_ex, extra_starts, size_t(B) * size_t(prm->n_extra) * 3 * sizeof(double), hipMemcpyHostToDevice, stream));
  SolveArgs a{};
  a.tables = d_tables;
  a.lengths = reinterpret_cast<const int32_t*>(base + o_len);
  a.mics = reinterpret_cast<const double*>(base + o_mic);
  a.calib = calib ? reinterpret_cast<const double*>(base + o_cal) : nullptr;
  a.weights = prm->weight_mode == PAL_SOLVE_W_ARRAY ? reinterpret_cast<const double*>(base + o_wt) : nullptr;
  a.extra = prm->n_extra > 0 ? reinterpret_cast<const double*>(base + o_ex) : nullptr;
  a.pair_idx = solve_idx;
  a.bw = reinterpret_cast<double2*>(base + o_bw);
  a.v = reinterpret_cast<double*>(base + o_v);
  a.starts = reinterpret_cast<double*>(base + o_st);
  a.frames = reinterpret_cast<SolveFrame*>(base + o_fr);
  a.results = reinterpret_cast<SolveStart*>(base + o_res);
  a.out = reinterpret_cast<pal_position_record*>(base + o_out);
  a.B = B; a.M = M; a.P = P; a.S = S;
  a.grid = prm->grid; a.n_extra = prm->n_extra; a.max_iter = prm->max_iter > 0 ? prm->max_iter : sv::kMaxIter; a.weight_mode = prm->weight_mode;
  a.fs = prm->fs; a.c = prm->c; a.buffer = prm->buffer;
  a.pair_weights = want_pw ? reinterpret_cast<double*>(base + o_pw) : nullptr;
  a.c2 = f_scale * f_scale; a.inv_c2 = 1.0 / a.c2; a.loss = loss;
  {
    ProfScope ps(this, "k_solve_prepare");
    k_solve_prepare<<<dim3(unsigned(B)), dim3(kPrepThreads), 0, stream>>>(a);
  }
  PAL_HIP(hipGetLastError());
  const dim3 lm_grid(unsigned(B * S));
  if (loss == sv::kLossLinear) {
    if (P <= 512) {           // a wavefront covers a small table (6 / 28 pairs at 4 / 8 microphones) in one to eight strides
      ProfScope ps(this, "k_solve_lm<64>");
      k_solve_lm<64><<<lm_grid, dim3(64), 0, stream>>>(a);
    } else {
      ProfScope ps(this, "k_solve_lm<256>");
      k_solve_lm<256><<<lm_grid, dim3(256), 0, stream>>>(a);
    }
  } else {
    ProfScope ps(this, P <= 512 ? "k_solve_lm<64, loss>" : "k_solve_lm<256, loss>");
    if (P <= 512) {
      if (loss == sv::kLossSoftL1) k_solve_lm<64, sv::kLossSoftL1><<<lm_grid, dim3(64), 0, stream>>>(a);
      else if (loss == sv::kLossHuber) k_solve_lm<64, sv::kLossHuber><<<lm_grid, dim3(64), 0, stream>>>(a);
      else k_solve_lm<64, sv::kLossCauchy><<<lm_grid, dim3(64), 0, stream>>>(a);
    } else {
      if (loss == sv::kLossSoftL1) k_solve_lm<256, sv::kLossSoftL1><<<lm_grid, dim3(256), 0, stream>>>(a);
      else if (loss == sv::kLossHuber) k_solve_lm<256, sv::kLossHuber><<<lm_grid, dim3(256), 0, stream>>>(a);
      else k_solve_lm<256, sv::kLossCauchy><<<lm_grid, dim3(256), 0, stream>>>(a);
    }
  }
  PAL_HIP(hipGetLastError());
  {
    ProfScope ps(this, "k_solve_pick");
    k_solve_pick<<<dim3(unsigned(B)), dim3(64), 0, stream>>>(a);
  }
  PAL_HIP(hipGetLastError());
  if (want_pw) {
    {
      ProfScope ps(this, "k_solve_weights");
      k_solve_weights<<<dim3(unsigned(B)), dim3(kWeightThreads), 0, stream>>>(a);
    }
    PAL_HIP(hipGetLastError());
    PAL_HIP(hipMemcpyAsync(pair_weights, base + o_pw, np * sizeof(double), hipMemcpyDeviceToHost, stream));
  }
  PAL_HIP(hipMemcpyAsync(out, base + o_out, size_t(B) * sizeof(pal_position_record), hipMemcpyDeviceToHost, stream));
  return check(hipStreamSynchronize(stream), "solve sync");
}

}  // namespace pal
