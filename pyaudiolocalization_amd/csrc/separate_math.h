// separate_math.h - the per-bin solve of the null-steering beamformer (k_separate in beamform.hip; specification:
// pyaudiolocalization_amd/beamform.py, solve_loaded) for host and device: the Cholesky factor of a Hermitian positive definite system
// of up to 8 unknowns and its two substitutions, on real and imaginary parts held in registers.  This file is the only place the
// operation order lives; it gives the specification's bits, so it is compiled with -ffp-contract=off wherever it is used (a product
// is rounded before it is added).  No HIP runtime calls; tests/host/test_separate_math.cpp runs it on the CPU against solve_loaded.
//
//   (G + delta I) z = y,   G Hermitian: dg[i] = G[i][i] + delta (real), the strict lower triangle in (gre, gim)[tri(i, j)], j < i
//
//   factor, j = 0 .. n-1:   s = dg[j];  for k = 0 .. j-1:  s = s - (Lre[j,k] Lre[j,k] + Lim[j,k] Lim[j,k])
//                           r[j] = 1 / sqrt(s)
//                           for i = j+1 .. n-1:  v = G[i,j];  for k = 0 .. j-1:  v = v - L[i,k] conj(L[j,k]);   L[i,j] = v r[j]
//   forward, i = 0 .. n-1:  v = y[i];  for k = 0 .. i-1:    v = v - L[i,k] z[k];         z[i] = v r[i]
//   back, i = n-1 .. 0:     v = z[i];  for k = i+1 .. n-1:  v = v - conj(L[k,i]) z[k];   z[i] = v r[i]
//
// with the complex products written out: (a + jb)(c + jd) = (ac - bd) + j(ad + bc), (a + jb) conj(c + jd) = (ac + bd) + j(bc - ad),
// conj(a + jb)(c + jd) = (ac + bd) + j(ad - bc), each bracket formed first and then subtracted from the running part.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define PAL_SEP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PAL_SEP_HD inline
#endif

namespace pal {

constexpr int kSeparateMax = 8;          // sources per frame: one solve cannot be split over passes

// the strict lower triangle, row by row: (1,0) (2,0) (2,1) (3,0) ...
PAL_SEP_HD constexpr int sep_tri(int i, int j) { return i * (i - 1) / 2 + j; }
constexpr int sep_tri_count(int n) { return n * (n - 1) / 2; }

// correctly rounded square root (device: the IEEE form whatever the file's flags say; host: the C++ operator)
PAL_SEP_HD double sep_sqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(x);
#else
  return std::sqrt(x);
#endif
}
PAL_SEP_HD double sep_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ddiv_rn(a, b);
#else
  return a / b;
#endif
}

// the n <= ST live unknowns of a tile of ST (n is uniform over a wavefront; every loop unrolls, so every index is a constant and the
// arrays stay in registers).  In place: the factor overwrites (gre, gim), z overwrites (yre, yim); dg is left as it came.
template <int ST>
PAL_SEP_HD void separate_solve(int n, const double (&dg)[ST], double (&gre)[sep_tri_count(ST) + 1], double (&gim)[sep_tri_count(ST) + 1],
                               double (&yre)[ST], double (&yim)[ST]) {
  double r[ST];
#pragma unroll
  for (int j = 0; j < ST; ++j) {
    if (j < n) {
      double s = dg[j];
#pragma unroll
      for (int k = 0; k < j; ++k) s = s - (gre[sep_tri(j, k)] * gre[sep_tri(j, k)] + gim[sep_tri(j, k)] * gim[sep_tri(j, k)]);
      r[j] = sep_div(1.0, sep_sqrt(s));
#pragma unroll
      for (int i = j + 1; i < ST; ++i) {
        if (i < n) {
          double vre = gre[sep_tri(i, j)], vim = gim[sep_tri(i, j)];
#pragma unroll
          for (int k = 0; k < j; ++k) {
            const double a = gre[sep_tri(i, k)], b = gim[sep_tri(i, k)], c = gre[sep_tri(j, k)], d = gim[sep_tri(j, k)];
            vre = vre - (a * c + b * d);
            vim = vim - (b * c - a * d);
          }
          gre[sep_tri(i, j)] = vre * r[j];
          gim[sep_tri(i, j)] = vim * r[j];
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < ST; ++i) {
    if (i < n) {
      double vre = yre[i], vim = yim[i];
#pragma unroll
      for (int k = 0; k < i; ++k) {
        const double a = gre[sep_tri(i, k)], b = gim[sep_tri(i, k)], c = yre[k], d = yim[k];
        vre = vre - (a * c - b * d);
        vim = vim - (a * d + b * c);
      }
      yre[i] = vre * r[i];
      yim[i] = vim * r[i];
    }
  }
#pragma unroll
  for (int i = ST - 1; i >= 0; --i) {
    if (i < n) {
      double vre = yre[i], vim = yim[i];
#pragma unroll
      for (int k = i + 1; k < ST; ++k) {
        if (k < n) {
          const double a = gre[sep_tri(k, i)], b = gim[sep_tri(k, i)], c = yre[k], d = yim[k];
          vre = vre - (a * c + b * d);
          vim = vim - (a * d - b * c);
        }
      }
      yre[i] = vre * r[i];
      yim[i] = vim * r[i];
    }
  }
}

}  // namespace pal
