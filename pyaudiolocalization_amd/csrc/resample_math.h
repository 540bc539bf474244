// resample_math.h - one output sample of signal_processing.resample_kaiser_best, for the kernel (resample.hip) and
// for the CPU (tests/host/test_resample_math.cpp): both compile THIS text.
//
// The NumPy specification makes one vectorised pass per filter tap over all outputs; read for one output sample t it is
//   t_reg = t * (1 / ratio);  n = int64(t_reg);  frac = scale * (t_reg - n)
//   left wing  : index_frac = frac * num_table, offset = int64(index_frac), eta = index_frac - offset,
//                taps = min(n + 1, (nwin - offset) // index_step);  tap i: weight = win[offset + i step] + eta * delta[...],
//                acc = acc + weight * x[n - i]
//   right wing : the same with scale - frac, min(n_orig - n - 1, ...) taps and x[n + 1 + i]
// in that order, every product rounded before it is added (build with -ffp-contract=off).  The specification also adds
// 0.0 * x[0] for the lanes whose wing has ended while another lane's goes on; that leaves a finite sum as it is, so
// stopping at the sample's own tap count gives the same bits.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PAL_RS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PAL_RS_HD inline
#endif

namespace pal {

struct alignas(16) ResampleTap {   // one table entry: win * ratio (or win) and its forward difference (0 for the last entry)
  double win, delta;
};

struct ResampleFilter {
  const ResampleTap* tab;   // nwin entries
  int nwin;                 // 64 zero crossings x 512 entries + 1
  int num_table;            // table entries per zero crossing (512)
  int index_step;           // int(scale * num_table); 0 for ratios below 1 / num_table (no taps at all, as NumPy's x // 0 = 0)
  double scale;             // min(1, ratio)
  double inv_ratio;         // 1.0 / ratio
};

// the table of a ratio from the filter's right wing: interp_win = win * ratio if ratio < 1 else win, interp_delta =
// np.diff(interp_win, append=interp_win[-1])
inline void resample_fill_table(const double* win, int nwin, double ratio, ResampleTap* tab) {
  for (int i = 0; i < nwin; ++i) tab[i].win = ratio < 1 ? win[i] * ratio : win[i];
  for (int i = 0; i < nwin; ++i) tab[i].delta = tab[i + 1 < nwin ? i + 1 : i].win - tab[i].win;
}

inline ResampleFilter resample_make_filter(const ResampleTap* tab, int nwin, int num_table, double ratio) {
  ResampleFilter f;
  f.tab = tab;
  f.nwin = nwin;
  f.num_table = num_table;
  f.scale = ratio < 1.0 ? ratio : 1.0;
  f.index_step = int(f.scale * double(num_table));
  f.inv_ratio = 1.0 / ratio;
  return f;
}

// most taps a wing can have (offset >= 0)
PAL_RS_HD int resample_wing_taps(const ResampleFilter& f) { return f.index_step > 0 ? f.nwin / f.index_step : 0; }

template <class Load>
PAL_RS_HD double resample_wing(const ResampleFilter& f, const Load& x, double frac, int64_t count, int64_t first, int sign, double acc) {
  const double index_frac = frac * double(f.num_table);
  const int64_t offset = int64_t(index_frac);
  const double eta = index_frac - double(offset);
  int64_t taps = f.index_step > 0 ? (int64_t(f.nwin) - offset) / f.index_step : 0;   // (nwin - offset > 0: frac <= scale <= 1)
  if (count < taps) taps = count;
  int64_t idx = offset, src = first;
  for (int64_t i = 0; i < taps; ++i) {
    const ResampleTap w = f.tab[idx];
    const double weight = w.win + eta * w.delta;
    acc = acc + weight * x(src);
    idx += f.index_step;
    src += sign;
  }
  return acc;
}

// x(i): sample i of the row, called for 0 <= i < n_orig only
template <class Load>
PAL_RS_HD double resample_sample(const ResampleFilter& f, const Load& x, int64_t n_orig, int64_t t) {
  const double t_reg = double(t) * f.inv_ratio;
  const int64_t n = int64_t(t_reg);
  if (n < 0 || n >= n_orig) return 0.0;     // never for t < int(n_orig * ratio); keeps every read inside the row
  const double frac = f.scale * (t_reg - double(n));
  double acc = 0.0;
  acc = resample_wing(f, x, frac, n + 1, n, -1, acc);                           // x[n], x[n - 1], ...
  acc = resample_wing(f, x, f.scale - frac, n_orig - n - 1, n + 1, +1, acc);    // x[n + 1], x[n + 2], ...
  return acc;
}

}  // namespace pal
