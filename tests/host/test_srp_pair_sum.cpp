// csrc/srp_cells.h on the CPU: srp_pair_sum, the body that carries k_srp_map, k_srp_zoom, k_srp_doa and k_srp_doa_zoom, with the steers
// and the terms those kernels give it, over small inputs from a file.  All files hold float64.
//   test_srp_pair_sum in.bin out.bin
//       in:  steer (0: distances to a point, 1: negated advances of a direction) term (0: nearest lag, 1: blended) M T N weighted fs c
//            mics[M][3] points[N][3] strips[P][2T+1] weights[P] (weighted != 0)
//       out: (power clipped)[N] at tid 0, then the same at tid 255
// Built with -ffp-contract=off (a product is rounded before it is added, like NumPy) and with the address and undefined-behaviour
// sanitizers: the strips, the weights and the 16 x 256 column are heap blocks of their exact size, so a read or write outside one is
// reported; the column is checked to be untouched outside the lane's own 16 entries.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "srp_cells.h"

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

// one point at lane `tid`: the kernels' steer for the geometry, the kernels' term
template <class TERM>
static int point(bool far, const vec& mics, int M, const double* wt, vec& column, int tid, const double* p, double& power, TERM term) {
  const double* m = mics.data();
  const int tiles = (M + pal::kPairTile - 1) / pal::kPairTile;
  if (far)
    return pal::srp_pair_sum(
        M, tiles, wt, column.data(), tid, power,
        [&](int i) { return -pal::srp_doa_advance(p[0], p[1], p[2], m[3 * i], m[3 * i + 1], m[3 * i + 2]); }, term);
  return pal::srp_pair_sum(
      M, tiles, wt, column.data(), tid, power, [&](int i) { return pal::srp_distance(p[0], p[1], p[2], m[3 * i], m[3 * i + 1], m[3 * i + 2]); },
      term);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
    return 2;
  }
  vec in;
  if (!read_doubles(argv[1], &in) || in.size() < 8) return 2;
  const bool far = in[0] != 0.0, blended = in[1] != 0.0, weighted = in[5] != 0.0;
  const int M = int(in[2]), T = int(in[3]), N = int(in[4]);
  const double fs = in[6], c = in[7];
  if (M < 2 || T < (blended ? 1 : 0) || N < 1) return 2;
  const int P = M * (M - 1) / 2, width = 2 * T + 1;
  if (in.size() != size_t(8 + 3 * M + 3 * N + P * width + (weighted ? P : 0))) return 2;
  const vec mics = slice(in, 8, size_t(3 * M)), points = slice(in, size_t(8 + 3 * M), size_t(3 * N));
  const vec strips = slice(in, size_t(8 + 3 * M + 3 * N), size_t(P) * size_t(width));
  const vec weights = weighted ? slice(in, size_t(8 + 3 * M + 3 * N + P * width), size_t(P)) : vec();
  const double* wt = weighted ? weights.data() : nullptr;
  const double* centre = strips.data() + T;
  const double mark = std::numeric_limits<double>::quiet_NaN();
  vec column(size_t(pal::kPairTile) * pal::kSrpThreads), out;
  for (const int tid : {0, pal::kSrpThreads - 1}) {
    for (int n = 0; n < N; ++n) {
      std::fill(column.begin(), column.end(), mark);
      double power = 0.0;
      const int clip = blended ? point(far, mics, M, wt, column, tid, &points[size_t(3 * n)], power, pal::SrpBlendTerm{centre, fs, c, T, width})
                               : point(far, mics, M, wt, column, tid, &points[size_t(3 * n)], power,
                                       pal::SrpNearestTerm{centre, fs, c, 1.0 / c, T, width});
      for (size_t at = 0; at < column.size(); ++at)
        if (int(at % pal::kSrpThreads) != tid && column[at] == column[at]) {
          std::printf("lane %d wrote column[%zu]\n", tid, at);
          return 3;
        }
      out.push_back(power);
      out.push_back(double(clip));
    }
  }
  if (!write_all(argv[2], out)) return 4;
  std::printf("ALL OK %d %d\n", N, P);
  return 0;
}
