// csrc/resample_math.h on the CPU: the per-sample function the resampling kernel runs, over one row.
//   test_resample_math win.bin num_table x.bin original_fs target_fs out.bin
// win.bin: the filter's right wing (float64), x.bin: the input row (float64); out.bin receives int(N * ratio) float64 samples.
// Built with -ffp-contract=off (products rounded before they are added, like NumPy) and with the address and undefined-behaviour
// sanitizers: the table and the row are heap blocks of their exact sizes, so a tap outside either one is reported.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "resample_math.h"

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

struct Row {
  const double* x;
  double operator()(int64_t i) const { return x[i]; }
};

int main(int argc, char** argv) {
  if (argc != 7) {
    std::fprintf(stderr, "usage: %s win.bin num_table x.bin original_fs target_fs out.bin\n", argv[0]);
    return 2;
  }
  std::vector<double> win, x;
  if (!read_doubles(argv[1], &win) || !read_doubles(argv[3], &x) || win.size() < 2 || x.empty()) {
    std::fprintf(stderr, "cannot read the inputs\n");
    return 2;
  }
  const int num_table = std::atoi(argv[2]);
  const double original_fs = std::atof(argv[4]), target_fs = std::atof(argv[5]);
  const double ratio = target_fs / original_fs;
  const int64_t n_orig = int64_t(x.size());
  const int64_t n_out = int64_t(double(n_orig) * ratio);
  if (!(ratio > 0) || n_out < 1) {
    std::fprintf(stderr, "nothing to resample\n");
    return 3;
  }
  std::vector<pal::ResampleTap> tab(win.size());
  pal::resample_fill_table(win.data(), int(win.size()), ratio, tab.data());
  const pal::ResampleFilter f = pal::resample_make_filter(tab.data(), int(tab.size()), num_table, ratio);
  std::vector<double> y(static_cast<size_t>(n_out));
  for (int64_t t = 0; t < n_out; ++t) y[size_t(t)] = pal::resample_sample(f, Row{x.data()}, n_orig, t);
  FILE* fp = std::fopen(argv[6], "wb");
  if (!fp || std::fwrite(y.data(), sizeof(double), y.size(), fp) != y.size()) return 4;
  std::fclose(fp);
  std::printf("ALL OK %lld\n", static_cast<long long>(n_out));
  return 0;
}
