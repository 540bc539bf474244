// sim_rows.h - the loader and the storer of the exact-length inverse DFT(2N) that sim.hip (multipath synthesis,
// fractional_delay) and beamform.hip (delay-and-sum) share: two real rows per complex transform, the fade window of
// signal_processing.py:75-79 and the rows' power-of-two exponents on the way out.
#pragma once
#include <cmath>

#include "conv_kernels.h"

namespace pal {

namespace {

// ------------------------------------------------------------------ multipath synthesis
struct SimLoader {
  static constexpr const char* kName = "SimLoader";
  const cd* X;            // base spectra [bases][H], H = N + 1, transform length n = 2N
  const double* delays;   // [rows][K] seconds
  const double* gains;    // [rows][K]
  int K, rows, rows_per_base, N, row0;   // row0: first row of this launch group
  double val;             // 1.0 / (2N * (1/fs)): numpy.fft.fftfreq spacing (signal_processing.py:70)
  const cd* w;
  const int* base_exp;    // [bases] exponent of each base signal (k_row_exponent): its spectrum goes in times 2^-e
  __device__ cd term(int r, unsigned kk, double f, bool nyquist, bool mirror) const {
    r += row0;
    if (r >= rows) return mk(0, 0);
    const int base = r / rows_per_base;
    cd x = X[size_t(base) * (N + 1) + kk];
    x = mk(ldexp(x.x, -base_exp[base]), ldexp(x.y, -base_exp[base]));
    double hx = 0, hy = 0;
    const double a = -6.283185307179586 * f;               // (-1j * 2 * np.pi * freqs) ...
    for (int p = 0; p < K; ++p) {
      double s, c;
      sincos(a * delays[size_t(r) * K + p], &s, &c);       // ... * delay
      const double g = gains[size_t(r) * K + p];
      hx += g * c;
      hy += g * s;
    }
    cd z = cmul(x, mk(hx, hy));
    if (nyquist) z.y = 0;                                   // only the real part of bin N survives .real
    if (mirror) z.y = -z.y;
    return z;
  }
  __device__ cd operator()(int g, unsigned j) const {
    const unsigned n = 2u * unsigned(N);
    if (j >= n) return mk(0, 0);
    const bool mirror = j > unsigned(N), nyq = j == unsigned(N);
    const unsigned kk = mirror ? n - j : j;
    const double f = nyq ? -double(N) * val : double(kk) * val;   // fftfreq: bin N carries -fs/2
    const cd z1 = term(2 * g, kk, f, nyq, mirror);
    const cd z2 = term(2 * g + 1, kk, f, nyq, mirror);
    return cmul(mk(z1.x - z2.y, z1.y + z2.x), w[j]);
  }
};

struct SimStorer {
  static constexpr const char* kName = "SimStorer";
  double* out;
  size_t stride;
  int rows, N, out_len, fl, row0;
  double step_in, step_out;   // 1/(fl-1), -1/(fl-1)  (np.linspace steps, signal_processing.py:77-78)
  const cd* w;
  const int* unexp;           // exponent of the base of row r (k_row_exponent), or null where the rows are normalised afterwards
  int rows_per_base;
  __device__ double fade(int j) const {
    if (j < fl) return fl == 1 ? 0.0 : (j == fl - 1 ? 1.0 : double(j) * step_in);
    if (j >= N - fl) {
      const int i = j - (N - fl);
      return fl == 1 ? 1.0 : (i == fl - 1 ? 0.0 : double(i) * step_out + 1.0);
    }
    return 1.0;
  }
  __device__ void operator()(int g, unsigned j, cd y) const {
    if (j >= unsigned(out_len)) return;
    const cd z = cmul(y, w[j]);
    const double f = fade(int(j));
    const int r = row0 + 2 * g;
    if (r < rows) out[size_t(r) * stride + j] = unexp ? ldexp(z.x * f, unexp[r / rows_per_base]) : z.x * f;
    if (r + 1 < rows) out[size_t(r + 1) * stride + j] = unexp ? ldexp(z.y * f, unexp[(r + 1) / rows_per_base]) : z.y * f;
  }
};

}  // namespace

}  // namespace pal
