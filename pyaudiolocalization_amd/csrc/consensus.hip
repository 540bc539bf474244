// consensus.hip - loop-closure consensus over K candidate peaks per pair (pal_tdoa_consensus*; specification:
// pyaudiolocalization_amd/consensus.py).
//
// The closure check (closure.hip) says which pairs of a TDOA table are wrong; here every pair brings K candidate lags and takes the one the
// other pairs' candidates agree with.  int32 arithmetic on array indices throughout, so the device equals the specification byte for byte.
//   k_consensus_prepare   one workgroup per (frame, microphone i): row i and column i of the dense signed candidate cube
//                         S[i][j][c] = lag({i,j}, c), S[j][i][c] = -lag({i,j}, c) in engine scratch, kAbsent for an absent candidate, for the
//                         diagonal and for the padding c >= K (the cube has KT = 1, 2, 4 or 8 >= K slots per pair).  A present candidate
//                         outside 0..2L-2, an absent candidate 0 and a gap in the prefix set the status bit kStInputBadCandidate (reported by
//                         pal_synchronize); an offending entry enters as lag 0, so no sum can overflow;
//   k_consensus_stage0    one workgroup per (frame, tile of kTile x kTile pairs, tiles on and above the diagonal), one lane per pair: the
//                         tile's i-rows and j-rows of S go through LDS in chunks of 256 / KT third microphones; per k the KT x KT differences
//                         S[i][k][a] - S[j][k][b] stay in registers while the pair's candidates are tested against them (kFar where a or b
//                         is absent - which also covers k = i and k = j); support[c] counts the k with a hit; sel_0 = the first maximum;
//   k_consensus_matrix    one workgroup per (frame, microphone i): row i of the antisymmetric matrix of the lags that a selection chooses;
//   k_consensus_round     closure's vote loop with KT tests per k: v[c] = #{k not in {i, j} : |A[i][k] - A[j][k] - lag(p, c)| <= tol}; writes
//                         the next selection (a pair keeps its candidate unless another has strictly more votes: then the first maximum)
//                         and / or the closure vote of the selection it read.  Jacobi: a round reads one selection buffer, writes another;
//   k_consensus_finish    one workgroup per frame: sel, table_out and the summary (closed triangles = a third of the sum of the votes).
// A call runs stage 0 and exactly `rounds` rounds: no early exit, no host read-back, no floating point, no waits between workgroups; a
// frame's results do not depend on which other frames share the call.
#include <climits>

#include "engine.h"

namespace pal {

constexpr int kCsTile = 16;                  // pairs per tile side: 256 lanes, one per pair
constexpr int kCsThreads = 256;
constexpr int kCsMaxMics = 256;
constexpr int kCsRowInts = 256;              // stage 0: ints of one cube row per LDS chunk = 256 / KT third microphones with KT slots each
// 16 B-aligned rows whose starts lie 4 banks apart: the sixteen j-rows a wavefront reads at one k (KT consecutive ints each, up to one
// 128-bit read) cover 16 x 4 = 64 distinct banks; the four i-rows of the wavefront are broadcast reads.  2 x 16 x 260 x 4 B = 33 280 B.
constexpr int kCsStride = kCsRowInts + 4;
constexpr int kCsMatStride = kCsMaxMics + 1; // rounds: closure's odd stride (one int per k).  2 x 16 x 257 x 4 B = 32 896 B
constexpr int32_t kAbsent = INT32_MIN;
constexpr int32_t kFar = 1 << 29;            // a difference with an absent side: |kFar - lag| > tol for every |lag| < 2^24 and tol <= 2^20
static_assert(kCsThreads == kCsTile * kCsTile && kCsThreads >= kCsMaxMics, "one lane per pair of a tile, one per microphone");

struct ConsensusArgs {
  const pal_pair_record* tables;   // [B][P] or nullptr (only table_out reads it)
  const int32_t* cand_k;           // [B][P][K]
  const double* cand_h;            // [B][P][K] or nullptr
  const int32_t* lengths;          // [B]
  int32_t* cube;                   // [B][M][M][KT]
  int32_t* lag;                    // [B][M][M]: the chosen lags of the selection that the next round reads
  const int32_t* sel_in;           // [B][P]: what k_consensus_matrix / k_consensus_round / k_consensus_finish read
  int32_t* sel_next;               // [B][P] or nullptr: k_consensus_stage0's and a round's result
  int32_t* votes_out;              // [B][P] or nullptr: closure votes of sel_in (k_consensus_round)
  const int32_t* sel_prev;         // [B][P]: the selection before the last round (finish: changed_last)
  const int32_t* votes_before;     // [B][P]: closure votes of candidate 0 / of the result (finish; nullptr without a summary)
  const int32_t* votes_after;
  int32_t* sel_out;                // the caller's outputs, each or nullptr
  pal_pair_record* table_out;
  pal_consensus_frame* summary;
  int* status;
  int B, M, P, K, tiles;
  int tol;
};

__device__ inline int cs_pair_row(int i, int M) { return i * M - i * (i + 1) / 2 - i - 1; }   // pair (i, j), i < j, is row cs_pair_row(i, M) + j

template <int KT>
__global__ __launch_bounds__(kCsThreads) void k_consensus_prepare(ConsensusArgs a) {
  const int b = blockIdx.x / a.M, i = blockIdx.x % a.M, M = a.M, K = a.K;
  int32_t* S = a.cube + size_t(b) * M * M * KT;
  const int lm1 = a.lengths[b] - 1;
  bool bad = false;
  for (int j = i + threadIdx.x; j < M; j += kCsThreads) {
    int32_t* fwd = S + (size_t(i) * M + j) * KT;
    if (j == i) {
#pragma unroll
      for (int c = 0; c < KT; ++c) fwd[c] = kAbsent;
      continue;
    }
    int32_t* rev = S + (size_t(j) * M + i) * KT;
    const int32_t* cand = a.cand_k + (size_t(b) * a.P + size_t(cs_pair_row(i, M) + j)) * K;
    bool ended = false;
#pragma unroll
    for (int c = 0; c < KT; ++c) {
      const int k = c < K ? cand[c] : -1;
      int lag = 0;
      bool present = true;
      if (k == -1) {
        if (c == 0) bad = true;           // candidate 0 must be there: it enters as lag 0
        else present = false;
        ended = true;
      } else {
        if (ended || k < 0 || k > 2 * lm1) bad = true;
        if (k >= 0 && k <= 2 * lm1) lag = k - lm1;
      }
      fwd[c] = present ? lag : kAbsent;
      rev[c] = present ? -lag : kAbsent;
    }
  }
  if (bad) atomicOr(a.status + kStInput, kStInputBadCandidate);
}

// the first c with the largest count among the present candidates (candidate 0 is always present in the cube)
template <int KT>
__device__ inline int cs_first_max(const int (&count)[KT], unsigned present) {
  int best = 0;
#pragma unroll
  for (int c = 1; c < KT; ++c)
    if (((present >> c) & 1u) && count[c] > count[best]) best = c;
  return best;
}

// uniform: tile t of a frame -> (ti, tj), tile row ti holds the tiles tj = ti .. tiles - 1
__device__ inline void cs_tile_of(int t, int tiles, int& ti, int& tj) {
  ti = 0;
  while (t >= tiles - ti) { t -= tiles - ti; ++ti; }
  tj = ti + t;
}

template <int KT>
__global__ __launch_bounds__(kCsThreads) void k_consensus_stage0(ConsensusArgs a) {
  __shared__ __attribute__((aligned(16))) int32_t rows_i[kCsTile * kCsStride];
  __shared__ __attribute__((aligned(16))) int32_t rows_j[kCsTile * kCsStride];
  constexpr int kChunk = kCsRowInts / KT;   // third microphones per LDS chunk
  constexpr int kUnroll = KT >= 4 ? 1 : 2;
  const int M = a.M, per_frame = a.tiles * (a.tiles + 1) / 2;
  const int b = blockIdx.x / per_frame, tid = threadIdx.x;
  int ti, tj;
  cs_tile_of(blockIdx.x % per_frame, a.tiles, ti, tj);
  const int32_t* S = a.cube + size_t(b) * M * M * KT;
  const int li = tid / kCsTile, lj = tid % kCsTile;
  const int i = ti * kCsTile + li, j = tj * kCsTile + lj;
  const bool active = i < j && j < M;
  const unsigned tol2 = 2u * unsigned(a.tol);
  int lo[KT], support[KT];
  unsigned present = 0;
#pragma unroll
  for (int c = 0; c < KT; ++c) {
    const int32_t v = active ? S[(size_t(i) * M + j) * KT + c] : kAbsent;
    if (v != kAbsent) present |= 1u << c;
    lo[c] = (v != kAbsent ? v : 0) - a.tol;
    support[c] = 0;
  }
  for (int k0 = 0; k0 < M; k0 += kChunk) {
    const int nk = M - k0 < kChunk ? M - k0 : kChunk, n = nk * KT;
    if (k0) __syncthreads();                // the previous chunk has been read
    for (int r = 0; r < kCsTile; ++r) {
      const int gi = ti * kCsTile + r, gj = tj * kCsTile + r;
      for (int x = tid; x < n; x += kCsThreads) {
        rows_i[r * kCsStride + x] = gi < M ? S[(size_t(gi) * M + k0) * KT + x] : kAbsent;
        rows_j[r * kCsStride + x] = gj < M ? S[(size_t(gj) * M + k0) * KT + x] : kAbsent;
      }
    }
    __syncthreads();
    if (!active) continue;
    const int32_t *ri = rows_i + li * kCsStride, *rj = rows_j + lj * kCsStride;
#pragma unroll kUnroll
    for (int kk = 0; kk < nk; ++kk) {
      int32_t si[KT], sj[KT], d[KT * KT];
#pragma unroll
      for (int c = 0; c < KT; ++c) {
        si[c] = ri[kk * KT + c];
        sj[c] = rj[kk * KT + c];
      }
#pragma unroll
      for (int x = 0; x < KT; ++x)
#pragma unroll
        for (int y = 0; y < KT; ++y) d[x * KT + y] = (si[x] == kAbsent || sj[y] == kAbsent) ? kFar : si[x] - sj[y];
#pragma unroll
      for (int c = 0; c < KT; ++c) {
        bool hit = false;
#pragma unroll
        for (int x = 0; x < KT * KT; ++x) hit |= unsigned(d[x] - lo[c]) <= tol2;   // |d - lag| <= tol
        support[c] += hit;
      }
    }
  }
  if (active) a.sel_next[size_t(b) * a.P + cs_pair_row(i, M) + j] = cs_first_max<KT>(support, present);
}

template <int KT>
__global__ __launch_bounds__(kCsThreads) void k_consensus_matrix(ConsensusArgs a) {
  const int b = blockIdx.x / a.M, i = blockIdx.x % a.M, M = a.M, j = threadIdx.x;
  if (j >= M) return;
  int lag = 0;
  if (j != i) {
    const int p = i < j ? cs_pair_row(i, M) + j : cs_pair_row(j, M) + i;
    const int c = a.sel_in[size_t(b) * a.P + p];
    lag = a.cube[((size_t(b) * M + i) * M + j) * KT + c];
  }
  a.lag[(size_t(b) * M + i) * M + j] = lag;
}

template <int KT>
__global__ __launch_bounds__(kCsThreads) void k_consensus_round(ConsensusArgs a) {
  __shared__ int32_t rows_i[kCsTile * kCsMatStride], rows_j[kCsTile * kCsMatStride];
  constexpr int kUnroll = KT >= 8 ? 2 : 4;
  const int M = a.M, per_frame = a.tiles * (a.tiles + 1) / 2;
  const int b = blockIdx.x / per_frame, tid = threadIdx.x;
  int ti, tj;
  cs_tile_of(blockIdx.x % per_frame, a.tiles, ti, tj);
  const int32_t* A = a.lag + size_t(b) * M * M;
  for (int r = 0; r < kCsTile; ++r) {
    const int gi = ti * kCsTile + r, gj = tj * kCsTile + r;
    for (int k = tid; k < M; k += kCsThreads) {
      rows_i[r * kCsMatStride + k] = gi < M ? A[size_t(gi) * M + k] : 0;
      rows_j[r * kCsMatStride + k] = gj < M ? A[size_t(gj) * M + k] : 0;
    }
  }
  __syncthreads();
  const int li = tid / kCsTile, lj = tid % kCsTile;
  const int i = ti * kCsTile + li, j = tj * kCsTile + lj;
  if (i >= j || j >= M) return;
  const int32_t* own = a.cube + ((size_t(b) * M + i) * M + j) * KT;
  const unsigned tol2 = 2u * unsigned(a.tol);
  int lo[KT], v[KT];
  unsigned present = 0;
#pragma unroll
  for (int c = 0; c < KT; ++c) {
    const int32_t s = own[c];
    if (s != kAbsent) present |= 1u << c;
    lo[c] = (s != kAbsent ? s : 0) - a.tol;
    v[c] = 0;
  }
  const int32_t *ri = rows_i + li * kCsMatStride, *rj = rows_j + lj * kCsMatStride;
#pragma unroll kUnroll
  for (int k = 0; k < M; ++k) {
    const int d = ri[k] - rj[k];
    const bool third = k != i && k != j;
#pragma unroll
    for (int c = 0; c < KT; ++c) v[c] += third && unsigned(d - lo[c]) <= tol2;
  }
  const size_t p = size_t(b) * a.P + cs_pair_row(i, M) + j;
  const int cur = a.sel_in[p];
  int vcur = 0;
#pragma unroll
  for (int c = 0; c < KT; ++c) vcur = c == cur ? v[c] : vcur;
  if (a.votes_out) a.votes_out[p] = vcur;
  if (a.sel_next) {
    const int best = cs_first_max<KT>(v, present);
    int vbest = 0;
#pragma unroll
    for (int c = 0; c < KT; ++c) vbest = c == best ? v[c] : vbest;
    a.sel_next[p] = vcur < vbest ? best : cur;
  }
}

__global__ __launch_bounds__(kCsThreads) void k_consensus_finish(ConsensusArgs a) {
  __shared__ int moved, changed, before, after;
  const int b = blockIdx.x, tid = threadIdx.x, P = a.P, K = a.K;
  if (tid == 0) moved = changed = before = after = 0;
  __syncthreads();
  int my_moved = 0, my_changed = 0, my_before = 0, my_after = 0;
  for (int p = tid; p < P; p += kCsThreads) {
    const size_t at = size_t(b) * P + p;
    const int c = a.sel_in[at];
    my_moved += c != 0;
    my_changed += c != a.sel_prev[at];
    if (a.votes_before) {
      my_before += a.votes_before[at];
      my_after += a.votes_after[at];
    }
    if (a.sel_out) a.sel_out[at] = c;
    if (a.table_out) {
      pal_pair_record rec = a.tables[at];                   // (the compiler keeps this local record in LDS: 8 192 of the kernel's 8 208 B.
      rec.k_sel = a.cand_k[at * K + c];                     //  Patching table_out in place instead leaves 16 B and measured slower,
      if (a.cand_h) rec.sel_height = a.cand_h[at * K + c];  //  0.246 against 0.144 ms for 16 frames x 256 microphones)
      if (c != 0) rec.branch |= PAL_BR_CONSENSUS;
      a.table_out[at] = rec;
    }
  }
  if (a.summary) {
    atomicAdd(&moved, my_moved);
    atomicAdd(&changed, my_changed);
    atomicAdd(&before, my_before);
    atomicAdd(&after, my_after);
    __syncthreads();
    if (tid == 0) {
      pal_consensus_frame s;
      s.moved = moved;
      s.closed_before = before / 3;       // every closed triangle votes for its three pairs
      s.closed_after = after / 3;
      s.changed_last = changed;
      a.summary[b] = s;
    }
  }
}

static size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

#define PAL_CS_LAUNCH(kernel, KT, grid)                                                                   \
  do {                                                                                                    \
    ProfScope ps(this, #kernel);                                                                          \
    switch (KT) {                                                                                         \
      case 1: kernel<1><<<dim3(unsigned(grid)), dim3(kCsThreads), 0, stream>>>(a); break;                 \
      case 2: kernel<2><<<dim3(unsigned(grid)), dim3(kCsThreads), 0, stream>>>(a); break;                 \
      case 4: kernel<4><<<dim3(unsigned(grid)), dim3(kCsThreads), 0, stream>>>(a); break;                 \
      default: kernel<8><<<dim3(unsigned(grid)), dim3(kCsThreads), 0, stream>>>(a); break;                \
    }                                                                                                     \
  } while (0)

int Engine::tdoa_consensus_dev(const pal_pair_record* d_tables, const int32_t* d_cand_k, const double* d_cand_h, int B, int M, int K,
                               const int32_t* lengths, int32_t tol, int32_t rounds, int32_t* d_sel, pal_pair_record* d_table_out,
                               pal_consensus_frame* d_summary) {
  PAL_TRY(consensus_check(B, M, K, lengths, tol, rounds));
  if (!d_cand_k) return fail(PAL_ERR_INVALID, "NULL buffer");
  if (!d_sel && !d_table_out && !d_summary) return fail(PAL_ERR_INVALID, "no output requested");
  if (d_table_out && !d_tables) return fail(PAL_ERR_INVALID, "table_out needs the input tables");
  const int P = M * (M - 1) / 2, tiles = (M + kCsTile - 1) / kCsTile;
  const int KT = K <= 1 ? 1 : (K <= 2 ? 2 : (K <= 4 ? 4 : 8));
  const int64_t tile_grid = int64_t(B) * (tiles * (tiles + 1) / 2);
  if (int64_t(B) * M > INT32_MAX || tile_grid > INT32_MAX) return fail(PAL_ERR_UNSUPPORTED, "%d frames x %d microphones is too many for one call", B, M);
  // one scratch block: [lengths | cube | chosen-lag matrices | three selections (candidate 0, and two that the rounds alternate) | votes before, after]
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off = align256(off + bytes); return at; };
  const size_t np = size_t(B) * size_t(P);
  const size_t o_len = take(size_t(B) * sizeof(int32_t));
  const size_t o_cube = take(size_t(B) * size_t(M) * size_t(M) * size_t(KT) * sizeof(int32_t));
  const size_t o_lag = take(size_t(B) * size_t(M) * size_t(M) * sizeof(int32_t));
  const size_t o_zero = take(np * sizeof(int32_t));
  const size_t o_sel0 = take(np * sizeof(int32_t));
  const size_t o_sel1 = take(np * sizeof(int32_t));
  const size_t o_vb = take(d_summary ? np * sizeof(int32_t) : 0);
  const size_t o_va = take(d_summary ? np * sizeof(int32_t) : 0);
  char* base = nullptr;
  PAL_TRY(scratch(kWsConsensus, off, &base));
  int* status = nullptr;
  PAL_TRY(status_words(&status));
  PAL_HIP(hipMemcpyAsync(base + o_len, lengths, size_t(B) * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  PAL_HIP(hipStreamSynchronize(stream));   // `lengths` is host memory
  PAL_HIP(hipMemsetAsync(base + o_zero, 0, np * sizeof(int32_t), stream));
  int32_t* zero = reinterpret_cast<int32_t*>(base + o_zero);
  int32_t* sel[2] = {reinterpret_cast<int32_t*>(base + o_sel0), reinterpret_cast<int32_t*>(base + o_sel1)};
  int32_t* vb = reinterpret_cast<int32_t*>(base + o_vb);
  int32_t* va = reinterpret_cast<int32_t*>(base + o_va);
  ConsensusArgs a{};
  a.tables = d_tables;
  a.cand_k = d_cand_k;
  a.cand_h = d_cand_h;
  a.lengths = reinterpret_cast<const int32_t*>(base + o_len);
  a.cube = reinterpret_cast<int32_t*>(base + o_cube);
  a.lag = reinterpret_cast<int32_t*>(base + o_lag);
  a.status = status;
  a.B = B; a.M = M; a.P = P; a.K = K; a.tiles = tiles;
  a.tol = tol;
  // one pass of the chosen-lag form over the selection `in`: the next selection and / or the closure votes of `in`
  auto pass = [&](const int32_t* in, int32_t* next, int32_t* votes) -> int {
    a.sel_in = in;
    a.sel_next = next;
    a.votes_out = votes;
    PAL_CS_LAUNCH(k_consensus_matrix, KT, B * M);
    PAL_HIP(hipGetLastError());
    PAL_CS_LAUNCH(k_consensus_round, KT, tile_grid);
    return check(hipGetLastError(), "consensus round launch");
  };
  PAL_CS_LAUNCH(k_consensus_prepare, KT, B * M);
  PAL_HIP(hipGetLastError());
  if (KT == 1) {                           // one candidate per pair: stage 0 has nothing to choose from
    PAL_HIP(hipMemsetAsync(sel[0], 0, np * sizeof(int32_t), stream));
  } else {
    a.sel_next = sel[0];
    ProfScope ps(this, "k_consensus_stage0");
    switch (KT) {
      case 2: k_consensus_stage0<2><<<dim3(unsigned(tile_grid)), dim3(kCsThreads), 0, stream>>>(a); break;
      case 4: k_consensus_stage0<4><<<dim3(unsigned(tile_grid)), dim3(kCsThreads), 0, stream>>>(a); break;
      default: k_consensus_stage0<8><<<dim3(unsigned(tile_grid)), dim3(kCsThreads), 0, stream>>>(a); break;
    }
  }
  PAL_HIP(hipGetLastError());
  if (d_summary) PAL_TRY(pass(zero, nullptr, vb));
  const int32_t* prev = zero;
  int cur = 0;
  for (int r = 0; r < rounds; ++r) {
    PAL_TRY(pass(sel[cur], sel[cur ^ 1], nullptr));
    prev = sel[cur];
    cur ^= 1;
  }
  if (d_summary) PAL_TRY(pass(sel[cur], nullptr, va));
  a.sel_in = sel[cur];
  a.sel_prev = prev;
  a.votes_before = d_summary ? vb : nullptr;
  a.votes_after = d_summary ? va : nullptr;
  a.sel_out = d_sel;
  a.table_out = d_table_out;
  a.summary = d_summary;
  {
    ProfScope ps(this, "k_consensus_finish");
    k_consensus_finish<<<dim3(unsigned(B)), dim3(kCsThreads), 0, stream>>>(a);
  }
  return check(hipGetLastError(), "consensus launch");
}

// the argument checks both forms share (everything but the buffers)
int Engine::consensus_check(int B, int M, int K, const int32_t* lengths, int32_t tol, int32_t rounds) {
  if (B < 1) return fail(PAL_ERR_INVALID, "need B >= 1");
  if (M < 3 || M > kCsMaxMics) return fail(PAL_ERR_INVALID, "the consensus takes 3..%d microphones (got %d)", kCsMaxMics, M);
  if (K < 1 || K > PAL_MAX_CANDIDATES) return fail(PAL_ERR_INVALID, "candidates per pair %d outside 1..%d", K, PAL_MAX_CANDIDATES);
  if (tol < 0 || tol > (1 << 20)) return fail(PAL_ERR_INVALID, "tol %d outside 0..2^20", tol);
  if (rounds < 0 || rounds > PAL_MAX_CONSENSUS_ROUNDS) return fail(PAL_ERR_INVALID, "rounds %d outside 0..%d", rounds, PAL_MAX_CONSENSUS_ROUNDS);
  if (!lengths) return fail(PAL_ERR_INVALID, "NULL buffer");
  for (int b = 0; b < B; ++b)
    if (lengths[b] < 1 || lengths[b] > (1 << 24)) return fail(PAL_ERR_INVALID, "frame %d: length %d outside 1..2^24", b, lengths[b]);
  return PAL_OK;
}

}  // namespace pal
