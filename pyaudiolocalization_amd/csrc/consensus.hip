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
//   k_consensus_stage0    one workgroup per (frame, tile of 16 x 16 pairs, tiles on and above the diagonal), one lane per pair: the
//                         tile's i-rows and j-rows of S go through LDS in chunks of 256 / KT third microphones; per k the KT x KT differences
//                         S[i][k][a] - S[j][k][b] stay in registers while the pair's candidates are tested against them (kFar where a or b
//                         is absent - which also covers k = i and k = j); support[c] counts the k with a hit; sel_0 = the first maximum;
//   k_consensus_matrix    one workgroup per (frame, microphone i): row i of the antisymmetric matrix of the lags that a selection chooses;
//   k_consensus_round     closure's vote loop (closure_tiles.h) with KT tests per k: v[c] = #{k not in {i, j} : |A[i][k] - A[j][k] - lag(p, c)|
//                         <= tol}; writes the next selection (a pair keeps its candidate unless another has strictly more votes: then the
//                         first maximum).  Jacobi: a round reads one selection buffer, writes another;
//   k_closure_votes       (closure.hip, with a summary) the closure votes of candidate 0's and of the result's chosen-lag matrices;
//   k_consensus_finish    one workgroup per frame: sel, table_out and the summary (closed triangles = a third of the sum of the votes).
// A call runs stage 0 and exactly `rounds` rounds: no early exit, no host read-back, no floating point, no waits between workgroups; a
// frame's results do not depend on which other frames share the call.
#include "closure_tiles.h"
#include "engine.h"

namespace pal {

constexpr int kCsRowInts = 256;              // stage 0: ints of one cube row per LDS chunk = 256 / KT third microphones with KT slots each
// 16 B-aligned rows whose starts lie 4 banks apart: the sixteen j-rows a wavefront reads at one k (KT consecutive ints each, up to one
// 128-bit read) cover 16 x 4 = 64 distinct banks; the four i-rows of the wavefront are broadcast reads.  2 x 16 x 260 x 4 B = 33 280 B.
constexpr int kCsStride = kCsRowInts + 4;
constexpr int32_t kAbsent = INT32_MIN;
constexpr int32_t kFar = 1 << 29;            // a difference with an absent side: |kFar - lag| > tol for every |lag| < 2^24 and tol <= 2^20

struct ConsensusArgs {
  const pal_pair_record* tables;   // [B][P] or nullptr (only table_out reads it)
  const int32_t* cand_k;           // [B][P][K]
  const double* cand_h;            // [B][P][K] or nullptr
  const int32_t* lengths;          // [B]
  int32_t* cube;                   // [B][M][M][KT]
  int32_t* lag;                    // [B][M][M]: the chosen lags of the selection that the next round reads
  const int32_t* votes_before;     // [B][P]: closure votes of candidate 0 / of the result (finish; nullptr without a summary)
  const int32_t* votes_after;
  int32_t* sel_out;                // the caller's outputs, each or nullptr
  pal_pair_record* table_out;
  pal_consensus_frame* summary;
  int* status;
  int M, P, K, tiles;
  int tol;
  // what the host sets from launch to launch
  const int32_t* sel_in;           // [B][P]: what k_consensus_matrix / k_consensus_round / k_consensus_finish read
  int32_t* sel_next;               // [B][P]: k_consensus_stage0's and a round's result
  const int32_t* sel_prev;         // [B][P]: the selection before the last round (finish: changed_last)
};

template <int KT>
__global__ __launch_bounds__(kTileThreads) void k_consensus_prepare(ConsensusArgs a) {
  const int b = blockIdx.x / a.M, i = blockIdx.x % a.M, M = a.M, K = a.K;
  int32_t* S = a.cube + size_t(b) * M * M * KT;
  const int lm1 = a.lengths[b] - 1;
  bool bad = false;
  for (int j = i + threadIdx.x; j < M; j += kTileThreads) {
    int32_t* fwd = S + (size_t(i) * M + j) * KT;
    if (j == i) {
#pragma unroll
      for (int c = 0; c < KT; ++c) fwd[c] = kAbsent;
      continue;
    }
    int32_t* rev = S + (size_t(j) * M + i) * KT;
    const int32_t* cand = a.cand_k + (size_t(b) * a.P + size_t(pair_row(i, M) + j)) * K;
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
        if (ended) bad = true;
        lag = lag_of_index(k, lm1, bad);
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

template <int KT>
__global__ __launch_bounds__(kTileThreads) void k_consensus_stage0(ConsensusArgs a) {
  __shared__ __attribute__((aligned(16))) int32_t rows_i[kPairTile * kCsStride];
  __shared__ __attribute__((aligned(16))) int32_t rows_j[kPairTile * kCsStride];
  constexpr int kChunk = kCsRowInts / KT;   // third microphones per LDS chunk
  constexpr int kUnroll = KT >= 4 ? 1 : 2;
  const int M = a.M, per_frame = a.tiles * (a.tiles + 1) / 2;
  const int b = blockIdx.x / per_frame, tid = threadIdx.x;
  int ti, tj;
  tile_of(blockIdx.x % per_frame, a.tiles, ti, tj);
  const int32_t* S = a.cube + size_t(b) * M * M * KT;
  const int li = tid / kPairTile, lj = tid % kPairTile;
  const int i = ti * kPairTile + li, j = tj * kPairTile + lj;
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
    for (int r = 0; r < kPairTile; ++r) {
      const int gi = ti * kPairTile + r, gj = tj * kPairTile + r;
      for (int x = tid; x < n; x += kTileThreads) {
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
  if (active) a.sel_next[size_t(b) * a.P + pair_row(i, M) + j] = cs_first_max<KT>(support, present);
}

template <int KT>
__global__ __launch_bounds__(kTileThreads) void k_consensus_matrix(ConsensusArgs a) {
  const int b = blockIdx.x / a.M, i = blockIdx.x % a.M, M = a.M, j = threadIdx.x;
  if (j >= M) return;
  int lag = 0;
  if (j != i) {
    const int p = i < j ? pair_row(i, M) + j : pair_row(j, M) + i;
    const int c = a.sel_in[size_t(b) * a.P + p];
    lag = a.cube[((size_t(b) * M + i) * M + j) * KT + c];
  }
  a.lag[(size_t(b) * M + i) * M + j] = lag;
}

template <int KT>
__global__ __launch_bounds__(kTileThreads) void k_consensus_round(ConsensusArgs a) {
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
  const int32_t* own = a.cube + ((size_t(b) * M + i) * M + j) * KT;
  int lo[KT], v[KT];
  unsigned present = 0;
#pragma unroll
  for (int c = 0; c < KT; ++c) {
    const int32_t s = own[c];
    if (s != kAbsent) present |= 1u << c;
    lo[c] = (s != kAbsent ? s : 0) - a.tol;
  }
  tile_votes<KT>(rows_i + li * kLagStride, rows_j + lj * kLagStride, M, j, lo, 2u * unsigned(a.tol), v);
  const size_t p = size_t(b) * a.P + pair_row(i, M) + j;
  const int cur = a.sel_in[p], best = cs_first_max<KT>(v, present);
  int vcur = 0, vbest = 0;
#pragma unroll
  for (int c = 0; c < KT; ++c) {
    vcur = c == cur ? v[c] : vcur;
    vbest = c == best ? v[c] : vbest;
  }
  a.sel_next[p] = vcur < vbest ? best : cur;
}

__global__ __launch_bounds__(kTileThreads) void k_consensus_finish(ConsensusArgs a) {
  __shared__ int moved, changed, before, after;
  const int b = blockIdx.x, tid = threadIdx.x, P = a.P, K = a.K;
  if (tid == 0) moved = changed = before = after = 0;
  __syncthreads();
  int my_moved = 0, my_changed = 0, my_before = 0, my_after = 0;
  for (int p = tid; p < P; p += kTileThreads) {
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

#define PAL_CS_LAUNCH(kernel, KT, grid)                                                                   \
  do {                                                                                                    \
    ProfScope ps(this, #kernel);                                                                          \
    switch (KT) {                                                                                         \
      case 1: kernel<1><<<dim3(unsigned(grid)), dim3(kTileThreads), 0, stream>>>(a); break;                 \
      case 2: kernel<2><<<dim3(unsigned(grid)), dim3(kTileThreads), 0, stream>>>(a); break;                 \
      case 4: kernel<4><<<dim3(unsigned(grid)), dim3(kTileThreads), 0, stream>>>(a); break;                 \
      default: kernel<8><<<dim3(unsigned(grid)), dim3(kTileThreads), 0, stream>>>(a); break;                \
    }                                                                                                     \
  } while (0)

int Engine::tdoa_consensus_dev(const pal_pair_record* d_tables, const int32_t* d_cand_k, const double* d_cand_h, int B, int M, int K,
                               const int32_t* lengths, int32_t tol, int32_t rounds, int32_t* d_sel, pal_pair_record* d_table_out,
                               pal_consensus_frame* d_summary) {
  PAL_TRY(consensus_check(B, M, K, lengths, tol, rounds));
  if (!d_cand_k) return fail(PAL_ERR_INVALID, "NULL buffer");
  if (!d_sel && !d_table_out && !d_summary) return fail(PAL_ERR_INVALID, "no output requested");
  if (d_table_out && !d_tables) return fail(PAL_ERR_INVALID, "table_out needs the input tables");
  const int P = M * (M - 1) / 2, tiles = (M + kPairTile - 1) / kPairTile;
  const int KT = K <= 1 ? 1 : (K <= 2 ? 2 : (K <= 4 ? 4 : 8));
  const int tile_grid = B * (tiles * (tiles + 1) / 2);   // fits: consensus_check
  // one scratch block: [lengths | cube | chosen-lag matrices | three selections (candidate 0, and two that the rounds alternate) | votes before, after]
  Carve c;
  const size_t np = size_t(B) * size_t(P);
  const size_t o_len = c.take(size_t(B) * sizeof(int32_t));
  const size_t o_cube = c.take(size_t(B) * size_t(M) * size_t(M) * size_t(KT) * sizeof(int32_t));
  const size_t o_lag = c.take(size_t(B) * size_t(M) * size_t(M) * sizeof(int32_t));
  const size_t o_zero = c.take(np * sizeof(int32_t));
  const size_t o_sel0 = c.take(np * sizeof(int32_t));
  const size_t o_sel1 = c.take(np * sizeof(int32_t));
  const size_t o_vb = c.take(d_summary ? np * sizeof(int32_t) : 0);
  const size_t o_va = c.take(d_summary ? np * sizeof(int32_t) : 0);
  char* base = nullptr;
  PAL_TRY(scratch(kWsConsensus, c.off, &base));
  int* status = nullptr;
  PAL_TRY(status_words(&status));
  PAL_TRY(upload_lengths(lengths, B, base + o_len));
  PAL_HIP(hipMemsetAsync(base + o_zero, 0, np * sizeof(int32_t), stream));
  int32_t* zero = reinterpret_cast<int32_t*>(base + o_zero);
  int32_t* sel[2] = {reinterpret_cast<int32_t*>(base + o_sel0), reinterpret_cast<int32_t*>(base + o_sel1)};
  int32_t* vb = d_summary ? reinterpret_cast<int32_t*>(base + o_vb) : nullptr;
  int32_t* va = d_summary ? reinterpret_cast<int32_t*>(base + o_va) : nullptr;
  ConsensusArgs a{d_tables, d_cand_k, d_cand_h, reinterpret_cast<const int32_t*>(base + o_len), reinterpret_cast<int32_t*>(base + o_cube),
                  reinterpret_cast<int32_t*>(base + o_lag), vb, va, d_sel, d_table_out, d_summary, status, M, P, K, tiles, tol};
  // the chosen-lag matrices of the selection `in`, then its closure votes (closure.hip) or, with `next`, the round that writes the next selection
  auto pass = [&](const int32_t* in, int32_t* next, int32_t* votes) -> int {
    a.sel_in = in;
    a.sel_next = next;
    PAL_CS_LAUNCH(k_consensus_matrix, KT, B * M);
    PAL_HIP(hipGetLastError());
    if (!next) return lag_votes(a.lag, B, M, tol, votes);
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
      case 2: k_consensus_stage0<2><<<dim3(unsigned(tile_grid)), dim3(kTileThreads), 0, stream>>>(a); break;
      case 4: k_consensus_stage0<4><<<dim3(unsigned(tile_grid)), dim3(kTileThreads), 0, stream>>>(a); break;
      default: k_consensus_stage0<8><<<dim3(unsigned(tile_grid)), dim3(kTileThreads), 0, stream>>>(a); break;
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
  {
    ProfScope ps(this, "k_consensus_finish");
    k_consensus_finish<<<dim3(unsigned(B)), dim3(kTileThreads), 0, stream>>>(a);
  }
  return check(hipGetLastError(), "consensus launch");
}

// the argument checks both forms share (everything but the buffers)
int Engine::consensus_check(int B, int M, int K, const int32_t* lengths, int32_t tol, int32_t rounds) {
  PAL_TRY(frames_check("consensus", B, M, lengths, tol));
  if (K < 1 || K > PAL_MAX_CANDIDATES) return fail(PAL_ERR_INVALID, "candidates per pair %d outside 1..%d", K, PAL_MAX_CANDIDATES);
  if (rounds < 0 || rounds > PAL_MAX_CONSENSUS_ROUNDS) return fail(PAL_ERR_INVALID, "rounds %d outside 0..%d", rounds, PAL_MAX_CONSENSUS_ROUNDS);
  return PAL_OK;
}

}  // namespace pal
