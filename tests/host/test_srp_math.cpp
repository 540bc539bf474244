// csrc/srp_math.h on the CPU: the functions the SRP kernels run, over small inputs from files.
//   test_srp_math geometry  in.bin out_points.bin out_lags.bin out_clip.bin
//       in.bin (float64): lo[3] hi[3] count[3] fs c T M mics[M][3]
//       -> points[G][3] float64, lags[G][P] float64 (the rounded lag as srp_lag returns it), clip[G][P] uint8
//   test_srp_math strips    in.bin out.bin
//       in.bin (float64): L T W P rows[P][2L-1]   -> strips[P][2T+1] float64
//   test_srp_math marks     in.bin out.bin
//       in.bin (float64): nx ny nz R power[nx][ny][nz]   -> marks[G] uint8
// Built with -ffp-contract=off (a product is rounded before it is added, like NumPy) and with the address and undefined-behaviour
// sanitizers: every input is a heap block of its exact size, so a read outside a row or a map is reported.
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

template <class T>
static bool write_all(const char* path, const std::vector<T>& v) {
  FILE* fp = std::fopen(path, "wb");
  if (!fp) return false;
  const bool ok = v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), fp) == v.size();
  return std::fclose(fp) == 0 && ok;
}

static int geometry(char** argv) {
  std::vector<double> in;
  if (!read_doubles(argv[2], &in) || in.size() < 13) return 2;
  const double *lo = &in[0], *hi = &in[3];
  const int count[3] = {int(in[6]), int(in[7]), int(in[8])};
  const double fs = in[9], c = in[10];
  const int T = int(in[11]), M = int(in[12]);
  if (in.size() != size_t(13 + 3 * M)) return 2;
  const std::vector<double> mics(in.begin() + 13, in.end());       // its own block of exactly M x 3
  const int G = count[0] * count[1] * count[2], P = M * (M - 1) / 2;
  double step[3];
  for (int a = 0; a < 3; ++a) step[a] = pal::srp_step(lo[a], hi[a], count[a]);
  const double inv_c = 1.0 / c;
  std::vector<double> points(size_t(G) * 3), lags(size_t(G) * size_t(P)), d(static_cast<size_t>(M));
  std::vector<unsigned char> clip(size_t(G) * size_t(P));
  for (int g = 0; g < G; ++g) {
    int ix, iy, iz;
    pal::srp_cell(g, count[1], count[2], ix, iy, iz);
    const double x = pal::srp_coord(lo[0], step[0], ix), y = pal::srp_coord(lo[1], step[1], iy), z = pal::srp_coord(lo[2], step[2], iz);
    points[size_t(g) * 3] = x;
    points[size_t(g) * 3 + 1] = y;
    points[size_t(g) * 3 + 2] = z;
    for (int m = 0; m < M; ++m) d[size_t(m)] = pal::srp_distance(x, y, z, mics[size_t(3 * m)], mics[size_t(3 * m + 1)], mics[size_t(3 * m + 2)]);
    size_t p = size_t(g) * size_t(P);
    for (int i = 0; i < M; ++i)
      for (int j = i + 1; j < M; ++j, ++p) {
        lags[p] = pal::srp_lag(d[size_t(i)], d[size_t(j)], fs, c, inv_c);
        clip[p] = pal::srp_clipped(lags[p], T) ? 1 : 0;
      }
  }
  if (!write_all(argv[3], points) || !write_all(argv[4], lags) || !write_all(argv[5], clip)) return 4;
  std::printf("ALL OK %d %d\n", G, P);
  return 0;
}

static int strips(char** argv) {
  std::vector<double> in;
  if (!read_doubles(argv[2], &in) || in.size() < 4) return 2;
  const int L = int(in[0]), T = int(in[1]), W = int(in[2]), P = int(in[3]), n = 2 * L - 1;
  if (in.size() != 4 + size_t(P) * size_t(n) || T < 0 || W < 0 || W > pal::kSrpMaxSmooth || T + W > L - 1) return 2;
  std::vector<double> out(size_t(P) * size_t(2 * T + 1));
  for (int p = 0; p < P; ++p) {
    const std::vector<double> row(in.begin() + 4 + long(p) * n, in.begin() + 4 + long(p + 1) * n);   // its own block of exactly n
    for (int s = -T; s <= T; ++s) out[size_t(p) * size_t(2 * T + 1) + size_t(T + s)] = pal::srp_smooth(row.data(), n, s, W);
  }
  if (!write_all(argv[3], out)) return 4;
  std::printf("ALL OK %d\n", P);
  return 0;
}

static int marks(char** argv) {
  std::vector<double> in;
  if (!read_doubles(argv[2], &in) || in.size() < 4) return 2;
  const int nx = int(in[0]), ny = int(in[1]), nz = int(in[2]), R = int(in[3]), G = nx * ny * nz;
  if (in.size() != 4 + size_t(G)) return 2;
  const std::vector<double> power(in.begin() + 4, in.end());
  std::vector<unsigned char> out(static_cast<size_t>(G));
  for (int g = 0; g < G; ++g) {
    int ix, iy, iz;
    pal::srp_cell(g, ny, nz, ix, iy, iz);
    out[size_t(g)] = pal::srp_is_peak(power.data(), nx, ny, nz, ix, iy, iz, R) ? 1 : 0;
  }
  if (!write_all(argv[3], out)) return 4;
  std::printf("ALL OK %d\n", G);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 6 && !std::strcmp(argv[1], "geometry")) return geometry(argv);
  if (argc == 4 && !std::strcmp(argv[1], "strips")) return strips(argv);
  if (argc == 4 && !std::strcmp(argv[1], "marks")) return marks(argv);
  std::fprintf(stderr, "usage: %s geometry in.bin points.bin lags.bin clip.bin | strips in.bin out.bin | marks in.bin out.bin\n", argv[0]);
  return 2;
}
