// csrc/separate_math.h on the CPU: separate_solve, the in-register Cholesky factor and solve of k_separate, over small systems from a
// file, at every tile that holds them.  All files hold float64.
//   test_separate_math in.bin out.bin
//       in:  n count, then per system dg[n] gre[T] gim[T] yre[n] yim[n], T = n (n - 1) / 2 (the strict lower triangle row by row)
//       out: for every tile ST of 1, 2, 4, 8 with ST >= n, per system zre[n] zim[n]
// Built with -ffp-contract=off (a product is rounded before it is added, like NumPy) and with the address and undefined-behaviour
// sanitizers.  The entries of a tile beyond the n live unknowns hold NaN: a result that read one of them would show it.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "separate_math.h"

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

template <int ST>
static void run(int n, int count, const double* sys, vec* out) {
  if (ST < n) return;
  const int T = n * (n - 1) / 2;
  const double mark = std::numeric_limits<double>::quiet_NaN();
  for (int c = 0; c < count; ++c, sys += 3 * n + 2 * T) {
    double dg[ST], gre[pal::sep_tri_count(ST) + 1], gim[pal::sep_tri_count(ST) + 1], yre[ST], yim[ST];
    for (int i = 0; i < ST; ++i) dg[i] = yre[i] = yim[i] = mark;
    for (int i = 0; i < pal::sep_tri_count(ST) + 1; ++i) gre[i] = gim[i] = mark;
    for (int i = 0; i < n; ++i) {
      dg[i] = sys[i];
      yre[i] = sys[n + 2 * T + i];
      yim[i] = sys[2 * n + 2 * T + i];
    }
    for (int i = 0; i < T; ++i) {                             // row by row is sep_tri's order at every tile
      gre[i] = sys[n + i];
      gim[i] = sys[n + T + i];
    }
    pal::separate_solve<ST>(n, dg, gre, gim, yre, yim);
    for (int i = 0; i < n; ++i) out->push_back(yre[i]);
    for (int i = 0; i < n; ++i) out->push_back(yim[i]);
  }
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
    return 2;
  }
  vec in;
  if (!read_doubles(argv[1], &in) || in.size() < 2) return 2;
  const int n = int(in[0]), count = int(in[1]);
  if (n < 1 || n > pal::kSeparateMax || count < 1) return 2;
  if (in.size() != size_t(2) + size_t(count) * size_t(3 * n + n * (n - 1))) return 2;
  vec out;
  run<1>(n, count, in.data() + 2, &out);
  run<2>(n, count, in.data() + 2, &out);
  run<4>(n, count, in.data() + 2, &out);
  run<8>(n, count, in.data() + 2, &out);
  if (!write_all(argv[2], out)) return 4;
  std::printf("ALL OK %d %d\n", n, count);
  return 0;
}
