// bootstrap.hip - the bootstrap significance test of utils.py:183-216 on the device.
//
// Shuffle s of pair (i, j) is a pure function of (seed, i, j, s, L, mode, block_size): a counter-based generator in exact
// 64-bit integer arithmetic, restated bit for bit by pyaudiolocalization_amd/bootstrap.py (the specification).  The shuffled
// rows of one round are gathered into an engine scratch slot, their spectra go to the tail of the spectra buffer behind the
// R original rows, and the round's pairs (i, R + c) run through the pair pipeline as they are (pair_correlations).
#include <cmath>

#include "bootstrap_map.h"
#include "engine.h"

namespace pal {

// bluestein.hip: a pair list -> the packed transforms of the pair pipeline
__global__ void k_pairs_to_quads(const int32_t* __restrict__ pairs, int64_t P, int R, int4* __restrict__ quads, int* __restrict__ status);

struct BootShuffle {
  const double* rows;        // source rows [R][L]; without a pair list: the one row that is shuffled
  const int32_t* pairs;      // [P][2] row indices, or nullptr (every shuffle keyed on (pi, pj))
  int R, L, S, mode, bs;
  int32_t pi, pj;
  int64_t g0;                // first shuffle of the launch: pair (g0 + c) / S, shuffle (g0 + c) % S; without pairs shuffle g0 + c
  uint64_t seed;
  double* out;               // [C][L]
  int32_t* round_pairs;      // [C][2] = (i, R + c) for the pair pipeline, or nullptr
  int* status;               // kStInputBadRow: a row index outside 0..R-1 (reported by pal_synchronize)
};

constexpr int kBootPerThread = 4;

// One shuffled row per blockIdx.x, 1024 output samples per blockIdx.y: a gather of the source row (it stays in L2: 353 KB at
// L = 44 100) with coalesced stores.  The key, the circular shift and the landing place of the short block are uniform per
// workgroup.
__global__ __launch_bounds__(256) void k_bootstrap_shuffle(BootShuffle a) {
  const int c = blockIdx.x;
  const int64_t g = a.g0 + c;
  int32_t i = a.pi, j = a.pj;
  int64_t s = g;
  const double* src = a.rows;
  if (a.pairs) {
    const int64_t p = g / a.S;
    s = g - p * a.S;
    i = a.pairs[2 * p];
    j = a.pairs[2 * p + 1];
    const bool bad = i < 0 || i >= a.R || j < 0 || j >= a.R;
    if (bad && blockIdx.y == 0 && threadIdx.x == 0 && a.status) atomicOr(a.status + kStInput, kStInputBadRow);
    if (i < 0 || i >= a.R) i = 0;
    if (j < 0 || j >= a.R) j = 0;
    src = a.rows + size_t(j) * size_t(a.L);
  }
  if (a.round_pairs && blockIdx.y == 0 && threadIdx.x == 0) {
    a.round_pairs[2 * c] = i;
    a.round_pairs[2 * c + 1] = a.R + c;
  }
  const boot::ShuffleMap map(boot::key_of(a.seed, i, j, s), a.mode, uint32_t(a.L), uint32_t(a.bs));
  double* dst = a.out + size_t(c) * size_t(a.L);
  const uint32_t t0 = blockIdx.y * (256u * kBootPerThread) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kBootPerThread; ++k) {
    const uint32_t t = t0 + 256u * k;
    if (t < map.L) dst[t] = src[map(t)];
  }
}

// peaks[g0 + c] = cmax of the round's record c (peaks[p][s] is flat index p * S + s)
__global__ __launch_bounds__(256) void k_bootstrap_scatter(const pal_pair_record* __restrict__ rec, int C, double* __restrict__ peaks) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < C) peaks[c] = rec[c].cmax;
}

static int check_boot_args(Engine* e, int L, int32_t mode, int32_t block_size, int64_t S) {
  if (L < 1) return e->fail(PAL_ERR_INVALID, "need L >= 1");
  if (L > (1 << 20)) return e->fail(PAL_ERR_UNSUPPORTED, "frame length %d exceeds 2^20", L);
  if (mode != PAL_BOOT_PERMUTATION && mode != PAL_BOOT_BLOCK && mode != PAL_BOOT_CIRCULAR)
    return e->fail(PAL_ERR_INVALID, "unknown bootstrap mode %d (0 permutation, 1 block, 2 circular)", mode);
  if (block_size < 1) return e->fail(PAL_ERR_INVALID, "block_size must be at least 1 (got %d)", block_size);
  if (S < 1) return e->fail(PAL_ERR_INVALID, "num_bootstrap must be at least 1");
  return PAL_OK;
}

int Engine::bootstrap_shuffle_dev(const double* d_row, int L, int32_t i, int32_t j, int32_t mode, int32_t block_size, uint64_t seed,
                                  int64_t s0, int32_t S, double* d_out) {
  PAL_TRY(check_boot_args(this, L, mode, block_size, S));
  if (i < 0 || j < 0 || s0 < 0) return fail(PAL_ERR_INVALID, "row indices and the first shuffle must be non-negative");
  constexpr int kMaxRows = 65536;   // rows per launch (a grid stays far below 2^32 threads)
  for (int32_t c0 = 0; c0 < S; c0 += kMaxRows) {
    const int C = S - c0 < kMaxRows ? S - c0 : kMaxRows;
    BootShuffle a{d_row, nullptr, 1, L, S, mode, block_size, i, j, s0 + c0, seed, d_out + size_t(c0) * size_t(L), nullptr, nullptr};
    k_bootstrap_shuffle<<<dim3(unsigned(C), unsigned((L + 1023) / 1024)), dim3(256), 0, stream>>>(a);
    PAL_HIP(hipGetLastError());
  }
  return PAL_OK;
}

// Shuffled rows per round: four launch groups of the pair pipeline (2 x pal_set_chunk / the automatic group size pairs each), at
// most about 1 GiB of shuffled rows plus their spectra, in whole launch groups where that bound holds one.
int Engine::bootstrap_round(const Plan& pl, int L) const {
  const long long per_row = 8ll * L + 16ll * (long long)pl.spec_stride();
  const long long cap = (1ll << 30) / per_row;
  const long long group = 2ll * pair_group(pl.n);
  long long C = 4 * group;
  if (C > cap) C = cap >= group ? cap / group * group : cap;
  return int(C < 2 ? 2 : C);
}

int Engine::bootstrap_peaks_dev(const double* d_rows, int R, int L, const int32_t* d_pairs, int64_t P, int32_t S, int32_t mode,
                                int32_t block_size, uint64_t seed, double* d_peaks) {
  PAL_TRY(check_boot_args(this, L, mode, block_size, S));
  if (R < 1 || P < 1) return fail(PAL_ERR_INVALID, "need R >= 1, P >= 1");
  if (P > (int64_t(1) << 40) / S) return fail(PAL_ERR_UNSUPPORTED, "%lld pairs x %d shuffles is too many", (long long)P, S);
  Plan* pl = nullptr;
  PAL_TRY(get_plan(2 * L - 1, L, 2 * L - 1, &pl));
  const int64_t total = P * int64_t(S);
  const int Cmax = int(total < bootstrap_round(*pl, L) ? total : bootstrap_round(*pl, L));
  if (int64_t(R) + Cmax > INT32_MAX / 2) return fail(PAL_ERR_UNSUPPORTED, "too many rows");
  const size_t ss = pl->spec_stride();
  const int rows = R + Cmax;
  cd* spectra = nullptr;
  double* shuffled = nullptr;
  char* pp = nullptr;
  int* status = nullptr;
  // spectra of the R rows, then of the round's shuffled rows; one non-zero flag per row behind them
  PAL_TRY(scratch(kWsSpectra, size_t(rows) * ss * sizeof(cd) + size_t(rows) * sizeof(int), &spectra));
  PAL_TRY(scratch(kWsBootRows, size_t(Cmax) * size_t(L) * sizeof(double), &shuffled));
  // the round's tables: [pair list (i, R + c) | packed transforms | records]
  const size_t quad_off = (size_t(2 * Cmax) * sizeof(int32_t) + 15) & ~size_t(15);
  const size_t rec_off = quad_off + size_t((Cmax + 1) / 2) * sizeof(int4);
  PAL_TRY(scratch(kWsBootRound, rec_off + size_t(Cmax) * sizeof(pal_pair_record), &pp));
  PAL_TRY(status_words(&status));
  int* nonzero = reinterpret_cast<int*>(spectra + size_t(rows) * ss);
  int32_t* round_pairs = reinterpret_cast<int32_t*>(pp);
  int4* quads = reinterpret_cast<int4*>(pp + quad_off);
  pal_pair_record* rec = reinterpret_cast<pal_pair_record*>(pp + rec_off);
  // default peak selection (median, no lag window); only cmax = np.max(corr) is read
  pal_phat_params prm{};
  prm.fs = 1000.0;
  prm.threshold_multiplier = 1.0;
  prm.max_expected_delay = NAN;
  prm.threshold_method = 0;
  prm.peak_distance = 1;
  prm.num_peaks = 1;
  PAL_TRY(forward_spectra(*pl, d_rows, size_t(L), R, L, spectra, nonzero));
  for (int64_t g0 = 0; g0 < total; g0 += Cmax) {
    const int C = int(total - g0 < Cmax ? total - g0 : Cmax);
    BootShuffle a{d_rows, d_pairs, R, L, S, mode, block_size, 0, 0, g0, seed, shuffled, round_pairs, status};
    k_bootstrap_shuffle<<<dim3(unsigned(C), unsigned((L + 1023) / 1024)), dim3(256), 0, stream>>>(a);
    PAL_HIP(hipGetLastError());
    PAL_TRY(forward_spectra(*pl, shuffled, size_t(L), C, L, spectra + size_t(R) * ss, nonzero + R));
    const int64_t ntr = (C + 1) / 2;
    k_pairs_to_quads<<<dim3(unsigned((ntr + 255) / 256)), dim3(256), 0, stream>>>(round_pairs, C, R + C, quads, status);
    PAL_HIP(hipGetLastError());
    PAL_TRY(pair_correlations(*pl, spectra, R + C, quads, C, L, prm, rec, nullptr, nullptr, nonzero));
    k_bootstrap_scatter<<<dim3(unsigned((C + 255) / 256)), dim3(256), 0, stream>>>(rec, C, d_peaks + g0);
    PAL_HIP(hipGetLastError());
  }
  return PAL_OK;
}

}  // namespace pal
