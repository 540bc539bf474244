// srp_math.h - the arithmetic of the steered-response power maps (srp.hip, srp_cells.h; specification: pyaudiolocalization_amd/srp.py) for host and
// device: the grid point, the distance, the lag with its clip test, the smoothing sum of a lag strip and the neighbourhood rule of the
// map's peaks.  Every function gives the specification's bits, so it is compiled with -ffp-contract=off wherever it is used: a product
// is rounded before it is added.  No HIP runtime calls; tests/host/test_srp_math.cpp, tests/host/test_srp_zoom.cpp (the zoom's
// interpolated term, boxes and stop decisions) and tests/host/test_srp_doa.cpp (the direction map: directions, advances, the wrapped
// peak rule, tangent bases and points) run it on the CPU against srp.py.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define PAL_SRP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PAL_SRP_HD inline
#endif

namespace pal {

constexpr int kSrpMaxSmooth = 32;        // largest half-width W of the triangular smoothing
constexpr int kSrpMaxCount = 1024;       // cells per axis
constexpr int64_t kSrpMaxCells = int64_t(1) << 24;
constexpr int kSrpMaxPeaks = 8, kSrpMaxRadius = 4;

// correctly rounded square root and quotient.  Device: __dsqrt_rn and __ddiv_rn are the IEEE forms whatever the file's flags say (the
// plain operators are the same under the default flags; these do not change with -ffast-math style options); host: the C++ operators.
PAL_SRP_HD double srp_sqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(x);
#else
  return std::sqrt(x);
#endif
}
PAL_SRP_HD double srp_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ddiv_rn(a, b);
#else
  return a / b;
#endif
}

// cell size of one axis, and the centre of cell i: lo + (i + 0.5) * step in that order
PAL_SRP_HD double srp_step(double lo, double hi, int count) { return srp_div(hi - lo, double(count)); }
PAL_SRP_HD double srp_coord(double lo, double step, int i) { return lo + (double(i) + 0.5) * step; }

// g = (ix * ny + iy) * nz + iz
PAL_SRP_HD void srp_cell(int g, int ny, int nz, int& ix, int& iy, int& iz) {
  iz = g % nz;
  const int t = g / nz;
  iy = t % ny;
  ix = t / ny;
}

PAL_SRP_HD double srp_distance(double x, double y, double z, double mx, double my, double mz) {
  const double dx = x - mx, dy = y - my, dz = z - mz;
  double q = dx * dx;
  q = q + dy * dy;
  q = q + dz * dz;
  return srp_sqrt(q);
}

// r = rint(((dj - di) * fs) / c), half to even, as a double.  inv_c = 1 / c: the product a * inv_c lies within 2^-50 |a / c| of the
// quotient, so wherever it is farther than kSrpNearHalf from a half-integer both round to the same integer (|a / c| < 2^26: a lag
// beyond that is clipped by either); only a product that close to a half-integer pays for the division.
constexpr double kSrpNearHalf = 1e-6;
PAL_SRP_HD double srp_lag(double di, double dj, double fs, double c, double inv_c) {
  const double a = (dj - di) * fs;
  const double t = a * inv_c;
  const double r = rint(t);
  if (fabs(t) < 67108864.0 && !(fabs(fabs(t - r) - 0.5) < kSrpNearHalf)) return r;
  return rint(srp_div(a, c));
}

// a term is clipped iff not |r| <= T, decided on the double (NaN and infinities are clipped)
PAL_SRP_HD bool srp_clipped(double r, int T) { return !(fabs(r) <= double(T)); }

// raw[u] = row[(-u) mod n] for |u| < n: the row has zero lag at index 0 and peaks at d_i - d_j; u counts d_j - d_i
PAL_SRP_HD int srp_row_index(int u, int n) { return u > 0 ? n - u : -u; }

// out[T + s] of a strip: sum over u = -W .. W of (W + 1 - |u|) * raw[s + u] in increasing u; the first product starts the sum
PAL_SRP_HD double srp_smooth(const double* row, int n, int s, int W) {
  double acc = double(1) * row[srp_row_index(s - W, n)];
  for (int u = -W + 1; u <= W; ++u) acc = acc + double(W + 1 - (u < 0 ? -u : u)) * row[srp_row_index(s + u, n)];
  return acc;
}

// cell g = (ix, iy, iz) of a map power[nx][ny][nz] is a peak iff it is not NaN and no cell of its (2R+1)^3 neighbourhood, cut at the
// grid's border, is higher, or equal with a lower linear index
PAL_SRP_HD bool srp_is_peak(const double* power, int nx, int ny, int nz, int ix, int iy, int iz, int R) {
  const int g = (ix * ny + iy) * nz + iz;
  const double v = power[g];
  if (!(v == v)) return false;
  const int x0 = ix - R < 0 ? 0 : ix - R, x1 = ix + R > nx - 1 ? nx - 1 : ix + R;
  const int y0 = iy - R < 0 ? 0 : iy - R, y1 = iy + R > ny - 1 ? ny - 1 : iy + R;
  const int z0 = iz - R < 0 ? 0 : iz - R, z1 = iz + R > nz - 1 ? nz - 1 : iz + R;
  for (int x = x0; x <= x1; ++x)
    for (int y = y0; y <= y1; ++y) {
      const int base = (x * ny + y) * nz;
      for (int z = z0; z <= z1; ++z) {
        const double o = power[base + z];
        if (o > v || (o == v && base + z < g)) return false;
      }
    }
  return true;
}

// the order of the peaks: power descending, then index ascending.  true iff (pa, ga) comes before (pb, gb)
PAL_SRP_HD bool srp_before(double pa, int ga, double pb, int gb) { return pa > pb || (pa == pb && ga < gb); }

// ---- the coarse-to-fine zoom (srp.zoom): the strip read at the fractional lag ----
constexpr int kSrpMaxZoomCells = 16, kSrpMaxZoomLevels = 16;   // cells per axis of a level; levels

// q = ((dj - di) * fs) / c, the correctly rounded quotient: its fraction is used, so there is no product with 1 / c here
PAL_SRP_HD double srp_zoom_quotient(double di, double dj, double fs, double c) { return srp_div((dj - di) * fs, c); }

// k = floor(q) as a double.  The term reads samples k and k + 1 of the centred strip, so it is clipped iff not -T <= k <= T - 1,
// decided on the double (NaN and infinities are clipped); int(k) is taken only after this test has passed
PAL_SRP_HD double srp_zoom_floor(double q) { return floor(q); }
PAL_SRP_HD bool srp_zoom_clipped(double k, int T) { return !(k >= double(-T) && k <= double(T - 1)); }

// s0 + f * (s1 - s0), f = q - k in [0, 1]: the product is rounded before the addition
PAL_SRP_HD double srp_blend(double s0, double s1, double f) { return s0 + f * (s1 - s0); }

// the term at a quotient that is not clipped, from row[-T .. T], the centre of pair p's strip (row = strips[p] + T)
PAL_SRP_HD double srp_zoom_read(const double* row, double q) {
  const double k = srp_zoom_floor(q);
  const int at = int(k);
  return srp_blend(row[at], row[at + 1], q - k);
}

// one term of a point's power; false: clipped, *v untouched.  The kernels take the same three steps through SrpBlendTerm (srp_cells.h)
PAL_SRP_HD bool srp_zoom_term(const double* row, int T, double di, double dj, double fs, double c, double* v) {
  const double q = srp_zoom_quotient(di, dj, fs, c);
  if (srp_zoom_clipped(srp_zoom_floor(q), T)) return false;
  *v = srp_zoom_read(row, q);
  return true;
}

// a level's box around its centre, and the next level's half-extent: one cell of this level, so the next box covers the best cell
// and half of each neighbour
PAL_SRP_HD void srp_zoom_box(double ctr, double half, double& lo, double& hi) {
  lo = ctr - half;
  hi = ctr + half;
}
PAL_SRP_HD double srp_zoom_next_half(double lo, double hi, int Z) { return srp_step(lo, hi, Z); }

// a seed with a negative index is absent; a level whose best cell has no index (every power NaN) stops the zoom
PAL_SRP_HD bool srp_zoom_absent(int seed_index) { return seed_index < 0; }
PAL_SRP_HD bool srp_zoom_stops(int best_index) { return best_index < 0; }

// ---- the direction map (srp.doa_map, srp.doa_peaks, srp.doa_zoom): a source far away in direction u, no sine and no square root
// per cell ----
constexpr int kSrpMaxDoaCount = 1024;    // azimuths, and elevations, of a direction grid

// g = ia * n_el + ie; the direction of cell (ia, ie) from the tables az[ia] = (ca, sa) and el[ie] = (ce, se): one rounded product each
PAL_SRP_HD void srp_doa_cell(int g, int n_el, int& ia, int& ie) {
  ie = g % n_el;
  ia = g / n_el;
}
PAL_SRP_HD void srp_doa_direction(double ca, double sa, double ce, double se, double& ux, double& uy, double& uz) {
  ux = ce * ca;
  uy = ce * sa;
  uz = se;
}

// how far the plane wave from direction u reaches microphone m before it reaches the origin: d_j - d_i = a_i - a_j, so the lag of pair
// (i, j) is srp_lag(a_j, a_i, ...) and the zoom's term srp_zoom_term(row, T, a_j, a_i, ...).  The kernels pass (-a_i, -a_j) in the
// near field's order instead (srp_cells.h): negation is exact, so (-a_j) - (-a_i) has the bits of a_i - a_j
PAL_SRP_HD double srp_doa_advance(double ux, double uy, double uz, double mx, double my, double mz) {
  double a = ux * mx;
  a = a + uy * my;
  a = a + uz * mz;
  return a;
}

// cell (ia, ie) of power[n_az][n_el] is a peak iff it is not NaN and no cell at offsets (da, de) in -R .. R is higher, or equal with a
// lower linear index.  Elevation is cut at the border; azimuth is taken mod n_az when wrap != 0 and cut otherwise.  With
// n_az < 2R + 1 a wrapped offset lands on a cell twice, or on the cell itself: neither changes the answer.
PAL_SRP_HD bool srp_doa_is_peak(const double* power, int n_az, int n_el, int wrap, int ia, int ie, int R) {
  const int g = ia * n_el + ie;
  const double v = power[g];
  if (!(v == v)) return false;
  const int e0 = ie - R < 0 ? 0 : ie - R, e1 = ie + R > n_el - 1 ? n_el - 1 : ie + R;
  for (int da = -R; da <= R; ++da) {
    int x = ia + da;
    if (wrap) {
      x %= n_az;
      if (x < 0) x += n_az;
    } else if (x < 0 || x > n_az - 1) {
      continue;
    }
    const int base = x * n_el;
    for (int e = e0; e <= e1; ++e) {
      const double o = power[base + e];
      if (o > v || (o == v && base + e < g)) return false;
    }
  }
  return true;
}

// |v| as the zoom takes it: q = x*x; q = q + y*y; q = q + z*z; sqrt(q)
PAL_SRP_HD double srp_doa_norm(double x, double y, double z) {
  double q = x * x;
  q = q + y * y;
  q = q + z * z;
  return srp_sqrt(q);
}

// the tangent basis of a level's centre u.  k is the coordinate axis of the smallest |u_k|, the lowest axis winning ties (a NaN is
// never smaller); e1 = (k x u) / |k x u|: two copies or negations and a zero, divided by their norm; e2 = u x e1, each component the
// difference of two rounded products, not normalised
PAL_SRP_HD int srp_doa_axis(double ux, double uy, double uz) {
  int k = 0;
  double m = fabs(ux);
  if (fabs(uy) < m) {
    k = 1;
    m = fabs(uy);
  }
  if (fabs(uz) < m) k = 2;
  return k;
}
PAL_SRP_HD void srp_doa_basis(const double u[3], double e1[3], double e2[3]) {
  const int k = srp_doa_axis(u[0], u[1], u[2]);
  double x, y, z;
  if (k == 0) {
    x = 0.0;
    y = -u[2];
    z = u[1];
  } else if (k == 1) {
    x = u[2];
    y = 0.0;
    z = -u[0];
  } else {
    x = -u[1];
    y = u[0];
    z = 0.0;
  }
  const double n = srp_doa_norm(x, y, z);
  e1[0] = srp_div(x, n);
  e1[1] = srp_div(y, n);
  e1[2] = srp_div(z, n);
  e2[0] = u[1] * e1[2] - u[2] * e1[1];
  e2[1] = u[2] * e1[0] - u[0] * e1[2];
  e2[2] = u[0] * e1[1] - u[1] * e1[0];
}

// the point of cell (i, j) of a level: u + off_i * e1, then + off_j * e2, then divided by its norm
PAL_SRP_HD void srp_doa_point(const double u[3], const double e1[3], const double e2[3], double off_i, double off_j, double v[3]) {
  for (int a = 0; a < 3; ++a) {
    double t = u[a] + off_i * e1[a];
    t = t + off_j * e2[a];
    v[a] = t;
  }
  const double n = srp_doa_norm(v[0], v[1], v[2]);
  for (int a = 0; a < 3; ++a) v[a] = srp_div(v[a], n);
}

}  // namespace pal
