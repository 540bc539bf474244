// csrc/srp_math.h on the CPU: the functions the zoom kernel (k_srp_zoom) runs, over small inputs from files.
//   test_srp_zoom pairs in.bin out.bin
//       in.bin (float64): fs c T N strip[2T+1] (di dj)[N]
//       -> per pair five float64: q, k, f = q - k, clipped (0 / 1), the term (0 where clipped)
//   test_srp_zoom level in.bin out.bin
//       in.bin (float64): fs c T M Z best ctr[3] half[3] mics[M][3] strips[P][2T+1]
//       -> float64: lo[3] hi[3] points[Z^3][3] terms[Z^3][P][5] (as above, pairs in row-major order) next_ctr[3] next_half[3]
//          absent(-1) absent(0) stops(-1) stops(0)
//          next_ctr is the centre of cell `best`
// Built with -ffp-contract=off (a product is rounded before it is added, like NumPy) and with the address and undefined-behaviour
// sanitizers: every strip is a heap block of its exact size, so a read outside a strip is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "srp_math.h"

static bool read_doubles(const char* path, std::vector<double>* out) {
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

static bool write_all(const char* path, const std::vector<double>& v) {
  FILE* fp = std::fopen(path, "wb");
  if (!fp) return false;
  const bool ok = v.empty() || std::fwrite(v.data(), sizeof(double), v.size(), fp) == v.size();
  return std::fclose(fp) == 0 && ok;
}

// the five figures of one term; `strip` is a block of exactly 2T + 1 samples
static void term(const std::vector<double>& strip, int T, double di, double dj, double fs, double c, std::vector<double>* out) {
  const double q = pal::srp_zoom_quotient(di, dj, fs, c);
  const double k = pal::srp_zoom_floor(q);
  const bool clipped = pal::srp_zoom_clipped(k, T);
  double v = 0.0;
  const bool kept = pal::srp_zoom_term(strip.data() + T, T, di, dj, fs, c, &v);
  if (kept == clipped) std::abort();                                 // the term and the clip test decide alike
  out->push_back(q);
  out->push_back(k);
  out->push_back(q - k);
  out->push_back(clipped ? 1.0 : 0.0);
  out->push_back(clipped ? 0.0 : v);
}

static int pairs(char** argv) {
  std::vector<double> in;
  if (!read_doubles(argv[2], &in) || in.size() < 4) return 2;
  const double fs = in[0], c = in[1];
  const int T = int(in[2]), N = int(in[3]);
  if (T < 1 || in.size() != size_t(4 + 2 * T + 1 + 2 * N)) return 2;
  const std::vector<double> strip(in.begin() + 4, in.begin() + 4 + 2 * T + 1);
  std::vector<double> out;
  for (int n = 0; n < N; ++n) term(strip, T, in[size_t(4 + 2 * T + 1 + 2 * n)], in[size_t(4 + 2 * T + 2 + 2 * n)], fs, c, &out);
  if (!write_all(argv[3], out)) return 4;
  std::printf("ALL OK %d\n", N);
  return 0;
}

static int level(char** argv) {
  std::vector<double> in;
  if (!read_doubles(argv[2], &in) || in.size() < 12) return 2;
  const double fs = in[0], c = in[1];
  const int T = int(in[2]), M = int(in[3]), Z = int(in[4]), best = int(in[5]);
  const double *ctr = &in[6], *half = &in[9];
  const int P = M * (M - 1) / 2, G = Z * Z * Z, width = 2 * T + 1;
  if (T < 1 || M < 2 || Z < 2 || Z > pal::kSrpMaxZoomCells || best < 0 || best >= G || in.size() != size_t(12 + 3 * M + P * width)) return 2;
  const std::vector<double> mics(in.begin() + 12, in.begin() + 12 + 3 * M);
  std::vector<std::vector<double>> strips;
  for (int p = 0; p < P; ++p) strips.emplace_back(in.begin() + 12 + 3 * M + long(p) * width, in.begin() + 12 + 3 * M + long(p + 1) * width);
  double lo[3], hi[3], step[3];
  std::vector<double> out;
  for (int a = 0; a < 3; ++a) {
    pal::srp_zoom_box(ctr[a], half[a], lo[a], hi[a]);
    step[a] = pal::srp_step(lo[a], hi[a], Z);
  }
  out.insert(out.end(), lo, lo + 3);
  out.insert(out.end(), hi, hi + 3);
  std::vector<double> pts(size_t(G) * 3), d(static_cast<size_t>(M));
  for (int g = 0; g < G; ++g) {
    int ix, iy, iz;
    pal::srp_cell(g, Z, Z, ix, iy, iz);
    pts[size_t(g) * 3] = pal::srp_coord(lo[0], step[0], ix);
    pts[size_t(g) * 3 + 1] = pal::srp_coord(lo[1], step[1], iy);
    pts[size_t(g) * 3 + 2] = pal::srp_coord(lo[2], step[2], iz);
  }
  out.insert(out.end(), pts.begin(), pts.end());
  for (int g = 0; g < G; ++g) {
    const double x = pts[size_t(g) * 3], y = pts[size_t(g) * 3 + 1], z = pts[size_t(g) * 3 + 2];
    for (int m = 0; m < M; ++m) d[size_t(m)] = pal::srp_distance(x, y, z, mics[size_t(3 * m)], mics[size_t(3 * m + 1)], mics[size_t(3 * m + 2)]);
    int p = 0;
    for (int i = 0; i < M; ++i)
      for (int j = i + 1; j < M; ++j, ++p) term(strips[size_t(p)], T, d[size_t(i)], d[size_t(j)], fs, c, &out);
  }
  for (int a = 0; a < 3; ++a) out.push_back(pts[size_t(best) * 3 + size_t(a)]);
  for (int a = 0; a < 3; ++a) out.push_back(pal::srp_zoom_next_half(lo[a], hi[a], Z));
  out.push_back(pal::srp_zoom_absent(-1) ? 1.0 : 0.0);
  out.push_back(pal::srp_zoom_absent(0) ? 1.0 : 0.0);
  out.push_back(pal::srp_zoom_stops(-1) ? 1.0 : 0.0);
  out.push_back(pal::srp_zoom_stops(0) ? 1.0 : 0.0);
  if (!write_all(argv[3], out)) return 4;
  std::printf("ALL OK %d %d\n", G, P);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "pairs")) return pairs(argv);
  if (argc == 4 && !std::strcmp(argv[1], "level")) return level(argv);
  std::fprintf(stderr, "usage: %s pairs in.bin out.bin | level in.bin out.bin\n", argv[0]);
  return 2;
}
