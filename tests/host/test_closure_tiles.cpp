// Host checks of csrc/closure_tiles.h, what the closure check and the consensus share: the pair index and the tile order against plain
// enumerations, the vote loop lane by lane against a triple loop that skips k = i and k = j, the index -> lag rule at its borders.
// Built and run by tests/test_host_closure_tiles.py (no GPU needed):
//   hipcc -O2 -I pyaudiolocalization_amd/csrc tests/host/test_closure_tiles.cpp -o /tmp/test_closure_tiles
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "closure_tiles.h"

using namespace pal;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void test_pair_row() {
  for (int M = 2; M <= 256; ++M) {
    int p = 0;
    for (int i = 0; i < M; ++i)
      for (int j = i + 1; j < M; ++j, ++p) CHECK(pair_row(i, M) + j == p, "M %d pair (%d, %d): row %d, want %d", M, i, j, pair_row(i, M) + j, p);
    CHECK(p == M * (M - 1) / 2, "M %d: %d pairs", M, p);
  }
  const int64_t M = 60000, i = M - 2;                    // i * M is past int32: the 64-bit form all_pairs_dev's pair order uses
  CHECK(pair_row(i, M) + (M - 1) == M * (M - 1) / 2 - 1, "64-bit pair_row: %lld", (long long)(pair_row(i, M) + (M - 1)));
}

static void test_tile_of() {
  for (int tiles = 1; tiles <= 16; ++tiles) {
    int t = 0;
    for (int ti = 0; ti < tiles; ++ti)
      for (int tj = ti; tj < tiles; ++tj, ++t) {
        int gi = -1, gj = -1;
        tile_of(t, tiles, gi, gj);
        CHECK(gi == ti && gj == tj, "tiles %d, tile %d: (%d, %d), want (%d, %d)", tiles, t, gi, gj, ti, tj);
      }
    CHECK(t == tiles * (tiles + 1) / 2, "tiles %d: %d tiles", tiles, t);
  }
}

static void test_lag_of_index() {
  for (int L : {1, 2, 12345, 1 << 24}) {
    const int lm1 = L - 1;
    const struct { int k, lag; bool bad; } cases[] = {{-1, 0, true}, {0, -lm1, false}, {2 * L - 2, lm1, false}, {2 * L - 1, 0, true}};
    for (const auto& c : cases) {
      bool bad = false;
      const int lag = lag_of_index(c.k, lm1, bad);
      CHECK(lag == c.lag && bad == c.bad, "L %d, k %d: lag %d bad %d", L, c.k, lag, int(bad));
    }
    bool bad = true;                                     // a good index leaves an earlier finding alone
    CHECK(lag_of_index(0, lm1, bad) == -lm1 && bad, "L %d: bad was cleared", L);
  }
}

// the vote of every pair of an antisymmetric matrix (rows of kLagStride ints, as in LDS) for KT candidate lags per pair: candidate 0 is
// the matrix entry itself (the closure vote), the others come from `other`
template <int KT, class Other>
static void votes_against_the_triple_loop(const std::vector<int32_t>& A, int M, int tol, Other other, const char* what) {
  for (int i = 0; i < M; ++i)
    for (int j = i + 1; j < M; ++j) {
      const int32_t *ri = A.data() + size_t(i) * kLagStride, *rj = A.data() + size_t(j) * kLagStride;
      int lag[KT], lo[KT], v[KT];
      for (int c = 0; c < KT; ++c) {
        lag[c] = c == 0 ? ri[j] : other();
        lo[c] = lag[c] - tol;
      }
      tile_votes<KT>(ri, rj, M, j, lo, 2u * unsigned(tol), v);
      for (int c = 0; c < KT; ++c) {
        int want = 0;
        for (int k = 0; k < M; ++k) {
          if (k == i || k == j) continue;
          const int64_t d = int64_t(ri[k]) - int64_t(rj[k]) - int64_t(lag[c]);
          want += (d < 0 ? -d : d) <= tol;
        }
        CHECK(v[c] == want, "%s KT %d, M %d, tol %d, pair (%d, %d), candidate %d: %d votes, want %d", what, KT, M, tol, i, j, c, v[c], want);
      }
    }
}

static void test_tile_votes() {
  std::mt19937 rng(5);
  std::uniform_int_distribution<int> lags(-40, 40);
  for (int M : {3, 16, 17, 33}) {
    std::vector<int32_t> A(size_t(M) * kLagStride, 0);
    for (int i = 0; i < M; ++i)
      for (int j = i + 1; j < M; ++j) {
        // half of the pairs consistent with positions on a line, so that triangles close; the others anywhere in +-40
        const int lag = (rng() & 1) ? 3 * (j - i) : lags(rng);
        A[size_t(i) * kLagStride + j] = lag;
        A[size_t(j) * kLagStride + i] = -lag;
      }
    for (int tol : {0, 1, 5}) {
      votes_against_the_triple_loop<1>(A, M, tol, [&] { return 0; }, "random");
      votes_against_the_triple_loop<4>(A, M, tol, [&] { return lags(rng); }, "random");
    }
  }
  // the largest lags and tolerance that the argument checks allow, in every combination of signs and zero over a triangle
  const int big = (1 << 24) - 1, value[3] = {-big, 0, big};
  int next = 0;
  for (int combo = 0; combo < 27; ++combo) {
    std::vector<int32_t> A(size_t(3) * kLagStride, 0);
    const int l01 = value[combo % 3], l02 = value[combo / 3 % 3], l12 = value[combo / 9];
    A[1] = l01; A[kLagStride] = -l01;
    A[2] = l02; A[2 * kLagStride] = -l02;
    A[kLagStride + 2] = l12; A[2 * kLagStride + 1] = -l12;
    for (int tol : {0, 1 << 20}) {
      votes_against_the_triple_loop<1>(A, 3, tol, [&] { return 0; }, "extreme");
      votes_against_the_triple_loop<4>(A, 3, tol, [&] { return value[next++ % 3]; }, "extreme");
    }
  }
}

int main() {
  test_pair_row();
  test_tile_of();
  test_lag_of_index();
  test_tile_votes();
  if (failures) {
    printf("%d FAILURES\n", failures);
    return 1;
  }
  printf("ALL OK\n");
  return 0;
}
