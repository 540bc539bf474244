// Host checks of the robust losses in csrc/solve_math.h (tests/test_host_solve_loss.py compiles this with the address and
// undefined-behaviour sanitizers and runs it).
//   selftest                       rho, rho' and rho' + 2 z rho'' of every loss against long-double evaluations (4 ulp), Huber's
//                                  two branches at the seam, loss_terms against the three single functions
//   lm <loss> <f_scale> <file>     [M, P, max_iter, lo3, hi3, x03, mics 3M, b P, w P] -> x, cost, iterations, stop rule of the
//                                  nineteen-sum iteration, the sums taken in pair order
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "solve_math.h"

namespace sv = pal::solve;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static const char* kNames[4] = {"linear", "soft_l1", "huber", "cauchy"};

// |got - want| in units of the float64 spacing at |want| (the smallest subnormal where want is below it)
static double ulps(double got, long double want) {
  const double w = double(fabsl(want));
  const double spacing = std::isinf(w) ? 0.0 : nextafter(w, INFINITY) - w;
  const long double err = fabsl((long double)got - want);
  return spacing > 0 ? double(err / (long double)spacing) : (err == 0 ? 0.0 : INFINITY);
}

static void want_ld(int loss, long double z, long double out[3]) {
  const long double one = 1.0L;
  if (loss == sv::kLossSoftL1) {
    const long double t = sqrtl(one + z);
    out[0] = 2.0L * z / (t + one);              // 2 (sqrt(1 + z) - 1) without the cancellation, which costs long double its digits too
    out[1] = one / t;
    out[2] = one / (t * (one + z));
  } else if (loss == sv::kLossHuber) {
    out[0] = z <= one ? z : 2.0L * sqrtl(z) - one;
    out[1] = z <= one ? one : one / sqrtl(z);
    out[2] = z <= one ? one : 0.0L;
  } else {
    out[0] = log1pl(z);
    out[1] = one / (one + z);
    out[2] = (one - z) / (one + z) / (one + z);
  }
}

template <int LOSS> static void check_loss() {
  const double zs[] = {0.0, 1e-300, 1e-16, 1e-8, 0.5, 1.0 - DBL_EPSILON, 1.0, 1.0 + DBL_EPSILON, 4.0, 1e8, 1e300};
  for (double z : zs) {
    long double want[3];
    want_ld(LOSS, (long double)z, want);
    const double got[3] = {sv::loss_rho<LOSS>(z), sv::loss_d1<LOSS>(z), sv::loss_curv<LOSS>(z)};
    for (int k = 0; k < 3; ++k) {
      const double u = ulps(got[k], want[k]);
      if (!(u <= 4.0)) { printf("FAIL %s z = %a: function %d = %a, want %.21Lg (%g ulp)\n", kNames[LOSS], z, k, got[k], want[k], u); ++fails; }
    }
    double rho, a, c;
    sv::loss_terms<LOSS>(z, &rho, &a, &c);
    CHECK(ulps(rho, want[0]) <= 4.0);
    CHECK(ulps(a, want[1]) <= 4.0);
    CHECK(ulps(c, want[2] > 0 ? want[2] : 0.0L) <= 4.0);     // clamped at zero
    CHECK(c >= 0.0 && a > 0.0 && a <= 1.0 && rho >= 0.0);
    CHECK(sv::loss_d1_of(LOSS, z) == got[1]);
  }
}

static int selftest() {
  check_loss<sv::kLossSoftL1>();
  check_loss<sv::kLossHuber>();
  check_loss<sv::kLossCauchy>();
  // Huber's seam: z = 1 belongs to the quadratic branch; both branches give the same value and slope there, the value does
  // not step down across it, and the curvature term switches from 1 to 0
  constexpr int H = sv::kLossHuber;
  const double below = 1.0 - DBL_EPSILON / 2, above = 1.0 + DBL_EPSILON;
  CHECK(sv::loss_rho<H>(1.0) == 1.0 && sv::loss_d1<H>(1.0) == 1.0 && sv::loss_curv<H>(1.0) == 1.0);
  CHECK(2.0 * sqrt(1.0) - 1.0 == sv::loss_rho<H>(1.0) && 1.0 / sqrt(1.0) == sv::loss_d1<H>(1.0));
  CHECK(sv::loss_rho<H>(below) == below && sv::loss_d1<H>(below) == 1.0 && sv::loss_curv<H>(below) == 1.0);
  CHECK(sv::loss_rho<H>(above) >= 1.0 && sv::loss_rho<H>(above) <= above);
  CHECK(sv::loss_d1<H>(above) <= 1.0 && sv::loss_d1<H>(above) >= 1.0 - DBL_EPSILON);
  CHECK(sv::loss_curv<H>(above) == 0.0);
  CHECK(sv::loss_rho<H>(4.0) == 3.0 && sv::loss_d1<H>(4.0) == 0.5);
  CHECK(sv::loss_d1_of(sv::kLossLinear, 7.0) == 1.0);
  printf(fails ? "%d FAILED\n" : "ALL OK\n", fails);
  return fails ? 1 : 0;
}

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

template <int LOSS>
static void run_lm(const std::vector<double>& v, double f_scale) {
  const int M = int(v[0]), P = int(v[1]), max_iter = int(v[2]);
  if (M < 2 || P != M * (M - 1) / 2 || v.size() != size_t(12 + 3 * M + 2 * P)) { printf("bad input\n"); exit(2); }
  const double *lo = &v[3], *hi = &v[6], *x0 = &v[9], *mics = &v[12], *b = mics + 3 * M, *w = b + P;
  std::vector<double> terms(size_t(M) * sv::kMicTerms);
  const double c2 = f_scale * f_scale, inv_c2 = 1.0 / c2;
  auto eval = [&](const double* x, double* out) {
    for (int m = 0; m < M; ++m) sv::mic_terms(x, mics + 3 * m, &terms[size_t(m) * sv::kMicTerms]);
    for (int q = 0; q < sv::kSumsLoss; ++q) out[q] = 0.0;
    int p = 0;
    for (int i = 0; i < M; ++i)
      for (int j = i + 1; j < M; ++j, ++p)
        sv::pair_accumulate_loss<LOSS>(out, &terms[size_t(i) * sv::kMicTerms], &terms[size_t(j) * sv::kMicTerms], b[p], w[p], inv_c2);
    out[15] = c2 * out[15];
  };
  double x[3], cost;
  int it, stop;
  sv::lm_solve<sv::kSumsLoss>(x0, lo, hi, max_iter, eval, x, &cost, &it, &stop);
  printf("%.17g %.17g %.17g %.17g %d %d\n", x[0], x[1], x[2], cost, it, stop);
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "selftest")) return selftest();
  if (argc == 5 && !strcmp(argv[1], "lm")) {
    const double f_scale = atof(argv[3]);
    const std::vector<double> v = read_all(argv[4]);
    if (v.size() < 12) { printf("bad input\n"); return 2; }
    if (!strcmp(argv[2], "soft_l1")) run_lm<sv::kLossSoftL1>(v, f_scale);
    else if (!strcmp(argv[2], "huber")) run_lm<sv::kLossHuber>(v, f_scale);
    else if (!strcmp(argv[2], "cauchy")) run_lm<sv::kLossCauchy>(v, f_scale);
    else { printf("unknown loss %s\n", argv[2]); return 2; }
    return 0;
  }
  printf("usage: %s selftest | lm <loss> <f_scale> <file>\n", argv[0]);
  return 2;
}
