// closure.hip - loop closure of TDOA tables on the device (pal_tdoa_closure*; specification: pyaudiolocalization_amd/closure.py).
//
// For three microphones x < y < z the lags of a consistent table close: lag_xy + lag_yz - lag_xz = 0 up to rounding.  A pair's vote is
// the number of third microphones whose triangle with it closes within `tol` samples.  Everything is int32 arithmetic on k_sel, so the
// device equals the specification bit for bit.  Three launches per call:
//   k_closure_prepare  one workgroup per (frame, microphone i): row i and column i of the frame's dense antisymmetric lag matrix
//                      A[i][j] = lag_ij, A[j][i] = -lag_ij, A[i][i] = 0 in engine scratch; a k_sel outside 0..2L-2 sets the status bit
//                      kStInputBadLag (reported by pal_synchronize) and enters the matrix as lag 0, so no sum can overflow;
//   k_closure_votes    one workgroup per (frame, tile of kTile x kTile pairs, tiles on and above the diagonal): the tile's i-rows and j-rows
//                      of A in LDS, one lane per pair, vote = #{k : |A[i][k] - A[j][k] - A[i][j]| <= tol} - 2 (k = i and k = j give
//                      exactly 0 and are counted by the loop, hence the 2);
//   k_closure_finish   one workgroup per frame: closed triangles per microphone (half the votes of its pairs), the weights, the summary.
// No floating-point atomics, no waits between workgroups; a frame's results do not depend on which other frames share the call.
#include <vector>

#include "engine.h"

namespace pal {

constexpr int kTile = 16;                 // pairs per tile side: 256 lanes, one per pair
constexpr int kClosureMaxMics = 256;
constexpr int kRowStride = kClosureMaxMics + 1;   // odd: the sixteen j-rows a wavefront reads at one k sit in sixteen banks
constexpr int kClosureThreads = 256;
static_assert(kClosureThreads == kTile * kTile && kClosureThreads >= kClosureMaxMics, "one lane per pair of a tile, one per microphone");

struct ClosureArgs {
  const pal_pair_record* tables;   // [B][P]
  const int32_t* lengths;          // [B]
  int32_t* lag;                    // [B][M][M]
  int32_t* votes;                  // [B][P]: the caller's buffer, or scratch
  int32_t* mic_closed;             // [B][M] or nullptr
  double* weights;                 // [B][P] or nullptr
  pal_closure_frame* summary;      // [B] or nullptr
  int* status;                     // engine status words
  int B, M, P, tiles;              // tiles per matrix side
  int tol, min_votes, weight_mode;
};

__device__ inline int pair_row(int i, int M) { return i * M - i * (i + 1) / 2 - i - 1; }   // pair (i, j), i < j, is row pair_row(i, M) + j

__global__ __launch_bounds__(kClosureThreads) void k_closure_prepare(ClosureArgs a) {
  const int b = blockIdx.x / a.M, i = blockIdx.x % a.M, M = a.M;
  const pal_pair_record* tab = a.tables + size_t(b) * a.P + pair_row(i, M);
  int32_t* A = a.lag + size_t(b) * M * M;
  const int lm1 = a.lengths[b] - 1;
  bool bad = false;
  for (int j = i + threadIdx.x; j < M; j += kClosureThreads) {
    int lag = 0;
    if (j > i) {
      const int k = tab[j].k_sel;
      if (k < 0 || k > 2 * lm1) bad = true;
      else lag = k - lm1;
      A[size_t(j) * M + i] = -lag;
    }
    A[size_t(i) * M + j] = lag;
  }
  if (bad) atomicOr(a.status + kStInput, kStInputBadLag);
}

__global__ __launch_bounds__(kClosureThreads) void k_closure_votes(ClosureArgs a) {
  __shared__ int32_t rows_i[kTile * kRowStride], rows_j[kTile * kRowStride];
  const int M = a.M, per_frame = a.tiles * (a.tiles + 1) / 2;
  const int b = blockIdx.x / per_frame;
  int t = blockIdx.x % per_frame, ti = 0;
  while (t >= a.tiles - ti) { t -= a.tiles - ti; ++ti; }          // uniform: tile row ti holds the tiles tj = ti .. tiles - 1
  const int tj = ti + t, tid = threadIdx.x;
  const int32_t* A = a.lag + size_t(b) * M * M;
  for (int r = 0; r < kTile; ++r) {
    const int gi = ti * kTile + r, gj = tj * kTile + r;
    for (int k = tid; k < M; k += kClosureThreads) {
      rows_i[r * kRowStride + k] = gi < M ? A[size_t(gi) * M + k] : 0;
      rows_j[r * kRowStride + k] = gj < M ? A[size_t(gj) * M + k] : 0;
    }
  }
  __syncthreads();
  const int li = tid / kTile, lj = tid % kTile;
  const int i = ti * kTile + li, j = tj * kTile + lj;
  if (i >= j || j >= M) return;
  const int32_t *ri = rows_i + li * kRowStride, *rj = rows_j + lj * kRowStride;
  const int aij = ri[j], tol = a.tol;
  int count = 0;
#pragma unroll 4
  for (int k = 0; k < M; ++k) {
    const int d = ri[k] - rj[k] - aij;
    count += (d < 0 ? -d : d) <= tol;
  }
  a.votes[size_t(b) * a.P + pair_row(i, M) + j] = count - 2;
}

__global__ __launch_bounds__(kClosureThreads) void k_closure_finish(ClosureArgs a) {
  __shared__ int closed_of[kClosureMaxMics];
  __shared__ int kept;
  const int b = blockIdx.x, tid = threadIdx.x, M = a.M, P = a.P;
  const int32_t* votes = a.votes + size_t(b) * P;
  if (tid == 0) kept = 0;
  if (tid < M) {                                        // kClosureThreads == kClosureMaxMics: one lane per microphone
    int sum = 0;
    for (int k = 0; k < M; ++k)
      if (k != tid) sum += k < tid ? votes[pair_row(k, M) + tid] : votes[pair_row(tid, M) + k];
    closed_of[tid] = sum / 2;                           // a closed triangle votes for two pairs of each of its microphones
    if (a.mic_closed) a.mic_closed[size_t(b) * M + tid] = sum / 2;
  }
  __syncthreads();
  int mine = 0;
  const double full = double(M - 2);
  for (int p = tid; p < P; p += kClosureThreads) {
    const int v = votes[p];
    const double w = v >= a.min_votes ? (a.weight_mode == PAL_CLOSURE_W_SOFT ? double(v) / full : 1.0) : 0.0;
    if (a.weights) a.weights[size_t(b) * P + p] = w;
    mine += w > 0.0;
  }
  if (mine) atomicAdd(&kept, mine);
  __syncthreads();
  if (tid == 0 && a.summary) {
    int total = 0, worst = 0;
    for (int m = 0; m < M; ++m) {
      total += closed_of[m];
      if (closed_of[m] < closed_of[worst]) worst = m;   // strict: the lowest index at ties
    }
    pal_closure_frame s;
    s.closed = total / 3;                               // every closed triangle is counted at its three microphones
    s.triangles = M * (M - 1) * (M - 2) / 6;
    s.kept_pairs = kept;
    s.worst_mic = worst;
    a.summary[b] = s;
  }
}

static size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

int Engine::tdoa_closure_dev(const pal_pair_record* d_tables, int B, int M, const int32_t* lengths, int32_t tol, int32_t min_votes,
                             int32_t weight_mode, int32_t* d_votes, int32_t* d_mic_closed, double* d_weights, pal_closure_frame* d_summary) {
  PAL_TRY(closure_check(B, M, lengths, tol, min_votes, weight_mode));
  if (!d_tables) return fail(PAL_ERR_INVALID, "NULL buffer");
  if (!d_votes && !d_mic_closed && !d_weights && !d_summary) return fail(PAL_ERR_INVALID, "no output requested");
  const int P = M * (M - 1) / 2, tiles = (M + kTile - 1) / kTile;
  const int64_t vote_grid = int64_t(B) * (tiles * (tiles + 1) / 2);
  if (int64_t(B) * M > INT32_MAX || vote_grid > INT32_MAX) return fail(PAL_ERR_UNSUPPORTED, "%d frames x %d microphones is too many for one call", B, M);
  // one scratch block: [lengths | lag matrices | votes (when the caller takes none)]
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off = align256(off + bytes); return at; };
  const size_t o_len = take(size_t(B) * sizeof(int32_t));
  const size_t o_lag = take(size_t(B) * size_t(M) * size_t(M) * sizeof(int32_t));
  const size_t o_votes = take(d_votes ? 0 : size_t(B) * size_t(P) * sizeof(int32_t));
  char* base = nullptr;
  PAL_TRY(scratch(kWsClosure, off, &base));
  int* status = nullptr;
  PAL_TRY(status_words(&status));
  PAL_HIP(hipMemcpyAsync(base + o_len, lengths, size_t(B) * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  PAL_HIP(hipStreamSynchronize(stream));   // `lengths` is host memory
  ClosureArgs a{};
  a.tables = d_tables;
  a.lengths = reinterpret_cast<const int32_t*>(base + o_len);
  a.lag = reinterpret_cast<int32_t*>(base + o_lag);
  a.votes = d_votes ? d_votes : reinterpret_cast<int32_t*>(base + o_votes);
  a.mic_closed = d_mic_closed;
  a.weights = d_weights;
  a.summary = d_summary;
  a.status = status;
  a.B = B; a.M = M; a.P = P; a.tiles = tiles;
  a.tol = tol; a.min_votes = min_votes; a.weight_mode = weight_mode;
  {
    ProfScope ps(this, "k_closure_prepare");
    k_closure_prepare<<<dim3(unsigned(B * M)), dim3(kClosureThreads), 0, stream>>>(a);
  }
  PAL_HIP(hipGetLastError());
  {
    ProfScope ps(this, "k_closure_votes");
    k_closure_votes<<<dim3(unsigned(vote_grid)), dim3(kClosureThreads), 0, stream>>>(a);
  }
  PAL_HIP(hipGetLastError());
  if (d_mic_closed || d_weights || d_summary) {
    ProfScope ps(this, "k_closure_finish");
    k_closure_finish<<<dim3(unsigned(B)), dim3(kClosureThreads), 0, stream>>>(a);
  }
  return check(hipGetLastError(), "closure launch");
}

// the argument checks both forms share (everything but the buffers)
int Engine::closure_check(int B, int M, const int32_t* lengths, int32_t tol, int32_t min_votes, int32_t weight_mode) {
  if (B < 1) return fail(PAL_ERR_INVALID, "need B >= 1");
  if (M < 3 || M > kClosureMaxMics) return fail(PAL_ERR_INVALID, "the closure check takes 3..%d microphones (got %d)", kClosureMaxMics, M);
  if (tol < 0 || tol > (1 << 20)) return fail(PAL_ERR_INVALID, "tol %d outside 0..2^20", tol);
  if (min_votes < 0) return fail(PAL_ERR_INVALID, "min_votes must not be negative");
  if (weight_mode != PAL_CLOSURE_W_MASK && weight_mode != PAL_CLOSURE_W_SOFT) return fail(PAL_ERR_INVALID, "unknown closure weight mode %d", weight_mode);
  if (!lengths) return fail(PAL_ERR_INVALID, "NULL buffer");
  for (int b = 0; b < B; ++b)
    if (lengths[b] < 1 || lengths[b] > (1 << 24)) return fail(PAL_ERR_INVALID, "frame %d: length %d outside 1..2^24", b, lengths[b]);
  return PAL_OK;
}

}  // namespace pal
