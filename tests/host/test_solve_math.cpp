// Host checks of csrc/solve_math.h (tests/test_host_solve.py compiles and runs this).
//   selftest                 the damped 3 x 3 solve against a long-double elimination, held coordinates, the box, the grid
//   npsum <file>             float64 array -> its sum in NumPy's pairwise order (%a)
//   pct <file>               float64 array -> the 75th percentile from the two order statistics (%a)
//   lm <file>                [M, P, max_iter, lo3, hi3, x03, mics 3M, b P, w P] -> x, cost, iterations, stop rule
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "solve_math.h"

namespace sv = pal::solve;

static std::vector<double> read_all(const char* path) {
  std::vector<double> v;
  FILE* f = fopen(path, "rb");
  if (!f) { printf("cannot open %s\n", path); exit(2); }
  double buf[4096];
  size_t n;
  while ((n = fread(buf, sizeof(double), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static void solve_ld(const long double m[3][3], const long double r[3], long double z[3]) {   // Gaussian elimination, partial pivoting
  long double a[3][4];
  for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) a[i][j] = m[i][j]; a[i][3] = r[i]; }
  for (int c = 0; c < 3; ++c) {
    int p = c;
    for (int i = c + 1; i < 3; ++i) if (fabsl(a[i][c]) > fabsl(a[p][c])) p = i;
    for (int j = 0; j < 4; ++j) std::swap(a[c][j], a[p][j]);
    for (int i = c + 1; i < 3; ++i) { const long double f = a[i][c] / a[c][c]; for (int j = c; j < 4; ++j) a[i][j] -= f * a[c][j]; }
  }
  for (int i = 2; i >= 0; --i) { long double s = a[i][3]; for (int j = i + 1; j < 3; ++j) s -= a[i][j] * z[j]; z[i] = s / a[i][i]; }
}

static int selftest() {
  unsigned long long seed = 12345;
  auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return double(seed >> 11) / 9007199254740992.0 - 0.5; };
  for (int trial = 0; trial < 2000; ++trial) {
    double j[5][3], h6[6] = {0, 0, 0, 0, 0, 0}, g[3] = {rnd(), rnd(), rnd()}, delta[3];
    for (auto& row : j) for (double& v : row) v = rnd();
    for (auto& row : j) { h6[0] += row[0] * row[0]; h6[1] += row[0] * row[1]; h6[2] += row[0] * row[2]; h6[3] += row[1] * row[1]; h6[4] += row[1] * row[2]; h6[5] += row[2] * row[2]; }
    const double d3[3] = {h6[0], h6[3], h6[5]};
    const double lam = trial % 3 == 0 ? 1e-3 : (trial % 3 == 1 ? 1.0 : 1e4);
    const bool held[3] = {(trial & 8) != 0, (trial & 16) != 0, (trial & 32) != 0};
    CHECK(sv::damped_step(h6, d3, g, lam, held, delta));
    long double m[3][3] = {{h6[0], h6[1], h6[2]}, {h6[1], h6[3], h6[4]}, {h6[2], h6[4], h6[5]}}, r[3], z[3];
    for (int k = 0; k < 3; ++k) { m[k][k] += (long double)lam * d3[k]; r[k] = -(long double)g[k]; }
    for (int k = 0; k < 3; ++k) if (held[k]) { for (int q = 0; q < 3; ++q) m[k][q] = m[q][k] = 0; m[k][k] = 1; r[k] = 0; }
    solve_ld(m, r, z);
    long double scale = 0;
    for (int k = 0; k < 3; ++k) scale = std::max(scale, fabsl(z[k]));
    for (int k = 0; k < 3; ++k) {
      if (held[k]) CHECK(delta[k] == 0.0);
      CHECK(fabsl(delta[k] - z[k]) <= 1e-10L * scale + 1e-300L);     // cond <= ~1e4 at lam = 1e-3 on five random rows
    }
  }
  {   // an indefinite matrix is refused
    const double h6[6] = {1, 2, 0, 1, 0, 1}, d3[3] = {1, 1, 1}, g[3] = {1, 1, 1};
    const bool held[3] = {false, false, false};
    double delta[3];
    CHECK(!sv::damped_step(h6, d3, g, 0.0, held, delta));
  }
  {   // box and grid
    const double mn[3] = {-1, 0, 2}, mx[3] = {1, 3, 2};
    double lo[3], hi[3], x[3];
    sv::box_from(mn, mx, 0.25, 5.0, lo, hi);
    CHECK(lo[0] == -7.0 && hi[0] == 7.0 && lo[2] == -4.0 && hi[2] == 8.0);
    sv::box_from(mn, mx, 2.5, 0.0, lo, hi);
    CHECK(lo[1] == -2.5 && hi[1] == 5.5);
    sv::grid_start(4 * 16 + 2 * 4 + 1 - 16 * 3, 4, lo, hi, x);   // cell (1, 2, 1)
    CHECK(x[0] == lo[0] + 1.5 * ((hi[0] - lo[0]) / 4) && x[1] == lo[1] + 2.5 * ((hi[1] - lo[1]) / 4) && x[2] == lo[2] + 1.5 * ((hi[2] - lo[2]) / 4));
  }
  printf(fails ? "FAILED\n" : "ALL OK\n");
  return fails ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "selftest")) return selftest();
  if (argc < 3) return 2;
  std::vector<double> v = read_all(argv[2]);
  if (!strcmp(argv[1], "npsum")) {
    std::vector<int32_t> off(sv::kNpMaxLeaves), len(sv::kNpMaxLeaves), prog(sv::kNpMaxProgram);
    std::vector<double> leaf(sv::kNpMaxLeaves);
    int np = 0;
    const int leaves = sv::np_plan(int64_t(v.size()), off.data(), len.data(), prog.data(), &np);
    auto get = [&](int64_t i) { return v[size_t(i)]; };
    for (int l = 0; l < leaves; ++l) leaf[l] = sv::np_leaf_sum(get, off[l], len[l]);
    printf("%a\n", sv::np_run_program(prog.data(), np, leaf.data()));
    return 0;
  }
  if (!strcmp(argv[1], "pct")) {
    double t = 0;
    const int64_t lo = sv::percentile75_rank(int64_t(v.size()), &t);
    std::sort(v.begin(), v.end());
    const double a = v[size_t(lo)], b = v[std::min(size_t(lo) + 1, v.size() - 1)];
    printf("%a\n", sv::percentile_lerp(a, b, t));
    return 0;
  }
  if (!strcmp(argv[1], "lm")) {
    const int M = int(v[0]), P = int(v[1]), max_iter = int(v[2]);
    const double *lo = &v[3], *hi = &v[6], *x0 = &v[9], *mics = &v[12], *b = mics + 3 * M, *w = b + P;
    std::vector<double> terms(size_t(M) * sv::kMicTerms);
    auto eval = [&](const double* x, double* out) {
      for (int m = 0; m < M; ++m) sv::mic_terms(x, mics + 3 * m, &terms[size_t(m) * sv::kMicTerms]);
      for (int q = 0; q < sv::kSums; ++q) out[q] = 0.0;
      int p = 0;
      for (int i = 0; i < M; ++i)
        for (int j = i + 1; j < M; ++j, ++p) sv::pair_accumulate(out, &terms[size_t(i) * sv::kMicTerms], &terms[size_t(j) * sv::kMicTerms], b[p], w[p]);
    };
    double x[3], cost;
    int it, stop;
    sv::lm_solve(x0, lo, hi, max_iter, eval, x, &cost, &it, &stop);
    printf("%.17g %.17g %.17g %.17g %d %d\n", x[0], x[1], x[2], cost, it, stop);
    return 0;
  }
  return 2;
}
