// closure.hip - loop closure of TDOA tables on the device (pal_tdoa_closure*; specification: pyaudiolocalization_amd/closure.py).
//
// For three microphones x < y < z the lags of a consistent table close: lag_xy + lag_yz - lag_xz = 0 up to rounding.  A pair's vote is
// the number of third microphones whose triangle with it closes within `tol` samples.  Everything is int32 arithmetic on k_sel, so the
// device equals the specification bit for bit.  Three launches per call:
//   k_closure_prepare  one workgroup per (frame, microphone i): row i and column i of the frame's dense antisymmetric lag matrix
//                      A[i][j] = lag_ij, A[j][i] = -lag_ij, A[i][i] = 0 in engine scratch; a k_sel outside 0..2L-2 sets the status bit
//                      kStInputBadLag (reported by pal_synchronize) and enters the matrix as lag 0, so no sum can overflow;
//   k_closure_votes    one workgroup per (frame, tile of 16 x 16 pairs, tiles on and above the diagonal): the tile's i-rows and j-rows of A
//                      in LDS, one lane per pair, vote = #{k not in {i, j} : |A[i][k] - A[j][k] - A[i][j]| <= tol} (closure_tiles.h, which
//                      the consensus shares; Engine::lag_votes launches it on any such matrices);
//   k_closure_finish   one workgroup per frame: closed triangles per microphone (half the votes of its pairs), the weights, the summary.
// No floating-point atomics, no waits between workgroups; a frame's results do not depend on which other frames share the call.
#include "closure_tiles.h"
#include "engine.h"

namespace pal {

struct ClosureArgs {
  const pal_pair_record* tables;   // [B][P]
  const int32_t* lengths;          // [B]
  int32_t* lag;                    // [B][M][M]
  const int32_t* votes;            // [B][P]: the caller's buffer, or scratch
  int32_t* mic_closed;             // [B][M] or nullptr
  double* weights;                 // [B][P] or nullptr
  pal_closure_frame* summary;      // [B] or nullptr
  int* status;                     // engine status words
  int M, P;
  int min_votes, weight_mode;
};

struct LagVotesArgs {
  const int32_t* lag;              // [B][M][M]: antisymmetric, zero diagonal
  int32_t* votes;                  // [B][P]
  int B, M, P, tiles;              // tiles per matrix side
  int tol;
};

__global__ __launch_bounds__(kTileThreads) void k_closure_prepare(ClosureArgs a) {
  const int b = blockIdx.x / a.M, i = blockIdx.x % a.M, M = a.M;
  const pal_pair_record* tab = a.tables + size_t(b) * a.P + pair_row(i, M);
  int32_t* A = a.lag + size_t(b) * M * M;
  const int lm1 = a.lengths[b] - 1;
  bool bad = false;
  for (int j = i + threadIdx.x; j < M; j += kTileThreads) {
    int lag = 0;
    if (j > i) {
      lag = lag_of_index(tab[j].k_sel, lm1, bad);
      A[size_t(j) * M + i] = -lag;
    }
    A[size_t(i) * M + j] = lag;
  }
  if (bad) atomicOr(a.status + kStInput, kStInputBadLag);
}

__global__ __launch_bounds__(kTileThreads) void k_closure_votes(LagVotesArgs a) {
  __shared__ int32_t rows_i[kPairTile * kLagStride], rows_j[kPairTile * kLagStride];
  const int M = a.M, per_frame = a.tiles * (a.tiles + 1) / 2;
  const int b = blockIdx.x / per_frame, tid = threadIdx.x;
  int ti, tj;
  tile_of(blockIdx.x % per_frame, a.tiles, ti, tj);
  load_lag_tile(a.lag + size_t(b) * M * M, M, ti, tj, rows_i, rows_j);
  __syncthreads();
  const int li = tid / kPairTile, lj = tid % kPairTile;
  const int i = ti * kPairTile + li, j = tj * kPairTile + lj;
  if (i >= j || j >= M) return;
  const int32_t *ri = rows_i + li * kLagStride, *rj = rows_j + lj * kLagStride;
  const int lo[1] = {ri[j] - a.tol};
  int v[1];
  tile_votes<1>(ri, rj, M, j, lo, 2u * unsigned(a.tol), v);
  a.votes[size_t(b) * a.P + pair_row(i, M) + j] = v[0];
}

__global__ __launch_bounds__(kTileThreads) void k_closure_finish(ClosureArgs a) {
  __shared__ int closed_of[kTileMaxMics];
  __shared__ int kept;
  const int b = blockIdx.x, tid = threadIdx.x, M = a.M, P = a.P;
  const int32_t* votes = a.votes + size_t(b) * P;
  if (tid == 0) kept = 0;
  if (tid < M) {                                        // kTileThreads == kTileMaxMics: one lane per microphone
    int sum = 0;
    for (int k = 0; k < M; ++k)
      if (k != tid) sum += k < tid ? votes[pair_row(k, M) + tid] : votes[pair_row(tid, M) + k];
    closed_of[tid] = sum / 2;                           // a closed triangle votes for two pairs of each of its microphones
    if (a.mic_closed) a.mic_closed[size_t(b) * M + tid] = sum / 2;
  }
  __syncthreads();
  int mine = 0;
  const double full = double(M - 2);
  for (int p = tid; p < P; p += kTileThreads) {
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

// closure votes of B antisymmetric M x M lag matrices with a zero diagonal (frames_check has seen that the grid fits an int32)
int Engine::lag_votes(const int32_t* d_lag, int B, int M, int tol, int32_t* d_votes) {
  const int tiles = (M + kPairTile - 1) / kPairTile;
  const LagVotesArgs a{d_lag, d_votes, B, M, M * (M - 1) / 2, tiles, tol};
  {
    ProfScope ps(this, "k_closure_votes");
    k_closure_votes<<<dim3(unsigned(B * (tiles * (tiles + 1) / 2))), dim3(kTileThreads), 0, stream>>>(a);
  }
  return check(hipGetLastError(), "closure votes launch");
}

int Engine::tdoa_closure_dev(const pal_pair_record* d_tables, int B, int M, const int32_t* lengths, int32_t tol, int32_t min_votes,
                             int32_t weight_mode, int32_t* d_votes, int32_t* d_mic_closed, double* d_weights, pal_closure_frame* d_summary) {
  PAL_TRY(closure_check(B, M, lengths, tol, min_votes, weight_mode));
  if (!d_tables) return fail(PAL_ERR_INVALID, "NULL buffer");
  if (!d_votes && !d_mic_closed && !d_weights && !d_summary) return fail(PAL_ERR_INVALID, "no output requested");
  const int P = M * (M - 1) / 2;
  // one scratch block: [lengths | lag matrices | votes (when the caller takes none)]
  Carve c;
  const size_t o_len = c.take(size_t(B) * sizeof(int32_t));
  const size_t o_lag = c.take(size_t(B) * size_t(M) * size_t(M) * sizeof(int32_t));
  const size_t o_votes = c.take(d_votes ? 0 : size_t(B) * size_t(P) * sizeof(int32_t));
  char* base = nullptr;
  PAL_TRY(scratch(kWsClosure, c.off, &base));
  int* status = nullptr;
  PAL_TRY(status_words(&status));
  PAL_TRY(upload_lengths(lengths, B, base + o_len));
  int32_t* votes = d_votes ? d_votes : reinterpret_cast<int32_t*>(base + o_votes);
  const ClosureArgs a{d_tables, reinterpret_cast<const int32_t*>(base + o_len), reinterpret_cast<int32_t*>(base + o_lag), votes,
                      d_mic_closed, d_weights, d_summary, status, M, P, min_votes, weight_mode};
  {
    ProfScope ps(this, "k_closure_prepare");
    k_closure_prepare<<<dim3(unsigned(B * M)), dim3(kTileThreads), 0, stream>>>(a);
  }
  PAL_HIP(hipGetLastError());
  PAL_TRY(lag_votes(a.lag, B, M, tol, votes));
  if (d_mic_closed || d_weights || d_summary) {
    ProfScope ps(this, "k_closure_finish");
    k_closure_finish<<<dim3(unsigned(B)), dim3(kTileThreads), 0, stream>>>(a);
  }
  return check(hipGetLastError(), "closure launch");
}

// what the closure check and the consensus (`what`) both ask of B frames of M microphones, their lengths (a host array) and the tolerance
int Engine::frames_check(const char* what, int B, int M, const int32_t* lengths, int32_t tol) {
  if (B < 1) return fail(PAL_ERR_INVALID, "need B >= 1");
  if (M < 3 || M > kTileMaxMics) return fail(PAL_ERR_INVALID, "the %s takes 3..%d microphones (got %d)", what, kTileMaxMics, M);
  if (tol < 0 || tol > (1 << 20)) return fail(PAL_ERR_INVALID, "tol %d outside 0..2^20", tol);
  if (!lengths) return fail(PAL_ERR_INVALID, "NULL buffer");
  for (int b = 0; b < B; ++b)
    if (lengths[b] < 1 || lengths[b] > (1 << 24)) return fail(PAL_ERR_INVALID, "frame %d: length %d outside 1..2^24", b, lengths[b]);
  const int tiles = (M + kPairTile - 1) / kPairTile;   // the grids: one workgroup per (frame, microphone) and per (frame, tile)
  if (int64_t(B) * M > INT32_MAX || int64_t(B) * (tiles * (tiles + 1) / 2) > INT32_MAX)
    return fail(PAL_ERR_UNSUPPORTED, "%d frames x %d microphones is too many for one call", B, M);
  return PAL_OK;
}

// the argument checks both forms share (everything but the buffers)
int Engine::closure_check(int B, int M, const int32_t* lengths, int32_t tol, int32_t min_votes, int32_t weight_mode) {
  PAL_TRY(frames_check("closure check", B, M, lengths, tol));
  if (min_votes < 0) return fail(PAL_ERR_INVALID, "min_votes must not be negative");
  if (weight_mode != PAL_CLOSURE_W_MASK && weight_mode != PAL_CLOSURE_W_SOFT) return fail(PAL_ERR_INVALID, "unknown closure weight mode %d", weight_mode);
  return PAL_OK;
}

}  // namespace pal
