// csrc/srp_math.h on the CPU: the functions the direction kernels (k_srp_doa, k_srp_doa_peaks, k_srp_doa_zoom) run, over small inputs
// from files.  All files hold float64.
//   test_srp_doa grid in.bin out.bin
//       in:  n_az n_el M fs c T wrap R az[n_az][2] el[n_el][2] mics[M][3] power[n_az][n_el]
//       out: directions[G][3] advances[G][M] (lag clipped)[G][P] (pairs row-major) marks[G]
//   test_srp_doa pairs in.bin out.bin
//       in:  fs c T N strip[2T+1] (aj ai)[N]
//       out: per pair seven: the map's lag and its clip flag; the zoom's q, k, f = q - k, clip flag and term (0 where clipped)
//   test_srp_doa level in.bin out.bin
//       in:  fs c T M Z half u[3] mics[M][3] strips[P][2T+1]
//       out: axis e1[3] e2[3] offsets[Z] points[Z^2][3] (q k f clipped term)[Z^2][P] (pairs row-major) next_half
// Built with -ffp-contract=off (a product is rounded before it is added, like NumPy) and with the address and undefined-behaviour
// sanitizers: every strip and table is a heap block of its exact size, so a read outside one is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "srp_math.h"

using vec = std::vector<double>;

static bool read_doubles(const char* path, vec* out) {
  FILE* fp = std::fopen(path, "rb");
  if (!fp) return false;
  std::fseek(fp, 0, SEEK_END);
  const long bytes = std::ftell(fp);
  std::fseek(fp, 0, SEEK_SET);
  out->resize(size_t(bytes) / sizeof(double));
  const size_t got = out->empty() ? 0 : std::fread(out->data(), sizeof(double), out->size(), fp);
  std::fclose(fp);
  return got == out->size();
}

static bool write_all(const char* path, const vec& v) {
  FILE* fp = std::fopen(path, "wb");
  if (!fp) return false;
  const bool ok = v.empty() || std::fwrite(v.data(), sizeof(double), v.size(), fp) == v.size();
  return std::fclose(fp) == 0 && ok;
}

static vec slice(const vec& in, size_t at, size_t count) { return vec(in.begin() + long(at), in.begin() + long(at + count)); }

// the zoom's five figures of one term; `strip` is a block of exactly 2T + 1 samples
static void zoom_term(const vec& strip, int T, double aj, double ai, double fs, double c, vec* out) {
  const double q = pal::srp_zoom_quotient(aj, ai, fs, c);
  const double k = pal::srp_zoom_floor(q);
  const bool clipped = pal::srp_zoom_clipped(k, T);
  double v = 0.0;
  const bool kept = pal::srp_zoom_term(strip.data() + T, T, aj, ai, fs, c, &v);
  if (kept == clipped) std::abort();                                 // the term and the clip test decide alike
  out->push_back(q);
  out->push_back(k);
  out->push_back(q - k);
  out->push_back(clipped ? 1.0 : 0.0);
  out->push_back(clipped ? 0.0 : v);
}

static void map_term(int T, double aj, double ai, double fs, double c, vec* out) {
  const double lag = pal::srp_lag(aj, ai, fs, c, 1.0 / c);
  out->push_back(lag);
  out->push_back(pal::srp_clipped(lag, T) ? 1.0 : 0.0);
}

static int grid(char** argv) {
  vec in;
  if (!read_doubles(argv[2], &in) || in.size() < 8) return 2;
  const int n_az = int(in[0]), n_el = int(in[1]), M = int(in[2]), T = int(in[5]), wrap = int(in[6]), R = int(in[7]);
  const double fs = in[3], c = in[4];
  if (n_az < 1 || n_el < 1 || M < 2 || T < 0 || R < 1) return 2;
  const int G = n_az * n_el;
  if (in.size() != size_t(8 + 2 * n_az + 2 * n_el + 3 * M + G)) return 2;
  const vec az = slice(in, 8, size_t(2 * n_az)), el = slice(in, size_t(8 + 2 * n_az), size_t(2 * n_el));
  const vec mics = slice(in, size_t(8 + 2 * n_az + 2 * n_el), size_t(3 * M)), power = slice(in, size_t(8 + 2 * n_az + 2 * n_el + 3 * M), size_t(G));
  vec dirs, adv, terms, marks;
  vec a(static_cast<size_t>(M));
  for (int g = 0; g < G; ++g) {
    int ia, ie;
    pal::srp_doa_cell(g, n_el, ia, ie);
    double ux, uy, uz;
    pal::srp_doa_direction(az[size_t(2 * ia)], az[size_t(2 * ia + 1)], el[size_t(2 * ie)], el[size_t(2 * ie + 1)], ux, uy, uz);
    dirs.insert(dirs.end(), {ux, uy, uz});
    for (int m = 0; m < M; ++m) a[size_t(m)] = pal::srp_doa_advance(ux, uy, uz, mics[size_t(3 * m)], mics[size_t(3 * m + 1)], mics[size_t(3 * m + 2)]);
    adv.insert(adv.end(), a.begin(), a.end());
    for (int i = 0; i < M; ++i)
      for (int j = i + 1; j < M; ++j) map_term(T, a[size_t(j)], a[size_t(i)], fs, c, &terms);
    marks.push_back(pal::srp_doa_is_peak(power.data(), n_az, n_el, wrap, ia, ie, R) ? 1.0 : 0.0);
  }
  vec out;
  for (const vec* v : {&dirs, &adv, &terms, &marks}) out.insert(out.end(), v->begin(), v->end());
  if (!write_all(argv[3], out)) return 4;
  std::printf("ALL OK %d %d\n", G, M);
  return 0;
}

static int pairs(char** argv) {
  vec in;
  if (!read_doubles(argv[2], &in) || in.size() < 4) return 2;
  const double fs = in[0], c = in[1];
  const int T = int(in[2]), N = int(in[3]);
  if (T < 1 || N < 0 || in.size() != size_t(4 + 2 * T + 1 + 2 * N)) return 2;
  const vec strip = slice(in, 4, size_t(2 * T + 1));
  vec out;
  for (int n = 0; n < N; ++n) {
    const double aj = in[size_t(4 + 2 * T + 1 + 2 * n)], ai = in[size_t(4 + 2 * T + 2 + 2 * n)];
    map_term(T, aj, ai, fs, c, &out);
    zoom_term(strip, T, aj, ai, fs, c, &out);
  }
  if (!write_all(argv[3], out)) return 4;
  std::printf("ALL OK %d\n", N);
  return 0;
}

static int level(char** argv) {
  vec in;
  if (!read_doubles(argv[2], &in) || in.size() < 9) return 2;
  const double fs = in[0], c = in[1], half = in[5];
  const int T = int(in[2]), M = int(in[3]), Z = int(in[4]);
  const double u[3] = {in[6], in[7], in[8]};
  const int P = M * (M - 1) / 2, G = Z * Z, width = 2 * T + 1;
  if (T < 1 || M < 2 || Z < 2 || Z > pal::kSrpMaxZoomCells || in.size() != size_t(9 + 3 * M + P * width)) return 2;
  const vec mics = slice(in, 9, size_t(3 * M));
  std::vector<vec> strips;
  for (int p = 0; p < P; ++p) strips.push_back(slice(in, size_t(9 + 3 * M) + size_t(p) * size_t(width), size_t(width)));
  double e1[3], e2[3];
  pal::srp_doa_basis(u, e1, e2);
  vec out;
  out.push_back(double(pal::srp_doa_axis(u[0], u[1], u[2])));
  out.insert(out.end(), e1, e1 + 3);
  out.insert(out.end(), e2, e2 + 3);
  const double step = pal::srp_step(-half, half, Z);
  for (int i = 0; i < Z; ++i) out.push_back(pal::srp_coord(-half, step, i));
  vec pts(size_t(G) * 3), a(static_cast<size_t>(M));
  for (int g = 0; g < G; ++g) pal::srp_doa_point(u, e1, e2, pal::srp_coord(-half, step, g / Z), pal::srp_coord(-half, step, g % Z), &pts[size_t(g) * 3]);
  out.insert(out.end(), pts.begin(), pts.end());
  for (int g = 0; g < G; ++g) {
    const double* v = &pts[size_t(g) * 3];
    for (int m = 0; m < M; ++m) a[size_t(m)] = pal::srp_doa_advance(v[0], v[1], v[2], mics[size_t(3 * m)], mics[size_t(3 * m + 1)], mics[size_t(3 * m + 2)]);
    int p = 0;
    for (int i = 0; i < M; ++i)
      for (int j = i + 1; j < M; ++j, ++p) zoom_term(strips[size_t(p)], T, a[size_t(j)], a[size_t(i)], fs, c, &out);
  }
  out.push_back(pal::srp_zoom_next_half(-half, half, Z));
  if (!write_all(argv[3], out)) return 4;
  std::printf("ALL OK %d %d\n", G, P);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "grid")) return grid(argv);
  if (argc == 4 && !std::strcmp(argv[1], "pairs")) return pairs(argv);
  if (argc == 4 && !std::strcmp(argv[1], "level")) return level(argv);
  std::fprintf(stderr, "usage: %s grid|pairs|level in.bin out.bin\n", argv[0]);
  return 2;
}
