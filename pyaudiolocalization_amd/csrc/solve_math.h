// solve_math.h - arithmetic of the batched position solve (solve.hip), host and device: the restatement in C++ of
// pyaudiolocalization_amd/solve.py (the specification; names and constants follow it).  tests/host/test_solve_math.cpp runs it
// on the host, tests/host/test_solve_loss.cpp the robust losses.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PAL_SOLVE_HD __host__ __device__
#else
#define PAL_SOLVE_HD
#endif

namespace pal {
namespace solve {

constexpr double kGtol = 1e-8, kXtol = 1e-13, kFtol = 1e-13, kLam0 = 1e-3, kLamMin = 1e-9, kLamMax = 1e12;
constexpr int kMaxIter = 200, kGrid = 4, kMaxGrid = 16, kMaxMics = 256;
enum Stop : int { kStopNone = 0, kStopGradient = 1, kStopStep = 2, kStopDecrease = 3, kStopDamping = 4, kStopCap = 5 };

// sums at a point: [0..5] JtJ, [6..11] second-order part of the Hessian (both xx, xy, xz, yy, yz, zz), [12..14] Jtr, [15] rtr
constexpr int kSums = 16;
// per microphone at a point: distance, unit vector, H = (I - u u^t) / d (six entries)
constexpr int kMicTerms = 10;

PAL_SOLVE_HD inline void mic_terms(const double x[3], const double m[3], double t[kMicTerms]) {
  const double dx = x[0] - m[0], dy = x[1] - m[1], dz = x[2] - m[2];
  const double d = sqrt(dx * dx + dy * dy + dz * dz);
  const double inv = d > 0 ? 1.0 / d : 0.0;
  const double ux = dx * inv, uy = dy * inv, uz = dz * inv;
  t[0] = d; t[1] = ux; t[2] = uy; t[3] = uz;
  t[4] = (1.0 - ux * ux) * inv; t[5] = (0.0 - ux * uy) * inv; t[6] = (0.0 - ux * uz) * inv;
  t[7] = (1.0 - uy * uy) * inv; t[8] = (0.0 - uy * uz) * inv; t[9] = (1.0 - uz * uz) * inv;
}

// one pair (i, j) with b = c td w and weight w
PAL_SOLVE_HD inline void pair_accumulate(double acc[kSums], const double* ti, const double* tj, double b, double w) {
  const double r = (tj[0] - ti[0]) * w - b;
  const double jx = (tj[1] - ti[1]) * w, jy = (tj[2] - ti[2]) * w, jz = (tj[3] - ti[3]) * w;
  const double rw = r * w;
  acc[0] += jx * jx; acc[1] += jx * jy; acc[2] += jx * jz; acc[3] += jy * jy; acc[4] += jy * jz; acc[5] += jz * jz;
#pragma unroll
  for (int q = 0; q < 6; ++q) acc[6 + q] += rw * (tj[4 + q] - ti[4 + q]);
  acc[12] += jx * r; acc[13] += jy * r; acc[14] += jz * r;
  acc[15] += r * r;
}

// ---- robust losses (solve.loss_terms): rho, rho' and rho' + 2 z rho'' at z = r^2 / C^2, SciPy's convention.  Written without
// cancellation at small z; every one is finite (or an exact zero) up to the largest float64.
enum Loss : int { kLossLinear = 0, kLossSoftL1 = 1, kLossHuber = 2, kLossCauchy = 3 };
// sums of a robust loss at a point: [0..5] sum c j j^t, [6..11] sum a r w (H_j - H_i), [12..14] the gradient sum a r j,
// [15] C^2 sum rho(z), [16..18] sum a j_k^2 (Marquardt's diagonal), with a = rho', c = max(rho' + 2 z rho'', 0)
constexpr int kSumsLoss = 19;

template <int LOSS> PAL_SOLVE_HD inline double loss_rho(double z) {
  if (LOSS == kLossSoftL1) return 2.0 * z / (sqrt(1.0 + z) + 1.0);       // 2 (sqrt(1 + z) - 1)
  if (LOSS == kLossHuber) return z <= 1.0 ? z : 2.0 * sqrt(z) - 1.0;
  if (LOSS == kLossCauchy) return log1p(z);
  return z;
}
template <int LOSS> PAL_SOLVE_HD inline double loss_d1(double z) {
  if (LOSS == kLossSoftL1) return 1.0 / sqrt(1.0 + z);
  if (LOSS == kLossHuber) return z <= 1.0 ? 1.0 : 1.0 / sqrt(z);
  if (LOSS == kLossCauchy) return 1.0 / (1.0 + z);
  return 1.0;
}
// rho' + 2 z rho'', not clamped: (1 + z)^-3/2, 1 | 0, (1 - z) / (1 + z)^2
template <int LOSS> PAL_SOLVE_HD inline double loss_curv(double z) {
  if (LOSS == kLossSoftL1) return 1.0 / sqrt(1.0 + z) / (1.0 + z);
  if (LOSS == kLossHuber) return z <= 1.0 ? 1.0 : 0.0;
  if (LOSS == kLossCauchy) { const double a = 1.0 / (1.0 + z); return (1.0 - z) * a * a; }
  return 1.0;
}
// all three with the shared square root or reciprocal computed once: (rho, a, c = max(curv, 0))
template <int LOSS> PAL_SOLVE_HD inline void loss_terms(double z, double* rho, double* a, double* c) {
  if (LOSS == kLossSoftL1) {
    const double t = sqrt(1.0 + z), ia = 1.0 / t;
    *rho = 2.0 * z / (t + 1.0); *a = ia; *c = ia / (1.0 + z);
  } else if (LOSS == kLossHuber) {
    const bool inner = z <= 1.0;
    const double t = sqrt(inner ? 1.0 : z);
    *rho = inner ? z : 2.0 * t - 1.0; *a = inner ? 1.0 : 1.0 / t; *c = inner ? 1.0 : 0.0;
  } else if (LOSS == kLossCauchy) {
    const double ia = 1.0 / (1.0 + z);
    *rho = log1p(z); *a = ia; *c = fmax((1.0 - z) * ia * ia, 0.0);
  } else {
    *rho = z; *a = 1.0; *c = 1.0;
  }
}
PAL_SOLVE_HD inline double loss_d1_of(int loss, double z) {
  return loss == kLossSoftL1 ? loss_d1<kLossSoftL1>(z) : loss == kLossHuber ? loss_d1<kLossHuber>(z) : loss == kLossCauchy ? loss_d1<kLossCauchy>(z) : 1.0;
}

// one pair under a robust loss; inv_c2 = 1 / C^2.  acc[15] collects rho(z): the caller scales the finished sum by C^2.
template <int LOSS>
PAL_SOLVE_HD inline void pair_accumulate_loss(double acc[kSumsLoss], const double* ti, const double* tj, double b, double w, double inv_c2) {
  const double r = (tj[0] - ti[0]) * w - b;
  const double jx = (tj[1] - ti[1]) * w, jy = (tj[2] - ti[2]) * w, jz = (tj[3] - ti[3]) * w;
  double rho, a, c;
  loss_terms<LOSS>((r * r) * inv_c2, &rho, &a, &c);
  const double ar = a * r, arw = ar * w;
  const double cx = c * jx, cy = c * jy, cz = c * jz;
  acc[0] += cx * jx; acc[1] += cx * jy; acc[2] += cx * jz; acc[3] += cy * jy; acc[4] += cy * jz; acc[5] += cz * jz;
#pragma unroll
  for (int q = 0; q < 6; ++q) acc[6 + q] += arw * (tj[4 + q] - ti[4 + q]);
  acc[12] += jx * ar; acc[13] += jy * ar; acc[14] += jz * ar;
  acc[15] += rho;
  acc[16] += a * (jx * jx); acc[17] += a * (jy * jy); acc[18] += a * (jz * jz);
}

// (H + lam diag(d3)) delta = -g on the free coordinates (held: delta = 0), LDLt without pivoting; false when a pivot is not positive
PAL_SOLVE_HD inline bool damped_step(const double h6[6], const double d3[3], const double g[3], double lam, const bool held[3], double delta[3]) {
  double m00 = h6[0] + lam * d3[0], m01 = h6[1], m02 = h6[2], m11 = h6[3] + lam * d3[1], m12 = h6[4], m22 = h6[5] + lam * d3[2];
  double r0 = -g[0], r1 = -g[1], r2 = -g[2];
  if (held[0]) { m00 = 1.0; m01 = 0.0; m02 = 0.0; r0 = 0.0; }
  if (held[1]) { m11 = 1.0; m01 = 0.0; m12 = 0.0; r1 = 0.0; }
  if (held[2]) { m22 = 1.0; m02 = 0.0; m12 = 0.0; r2 = 0.0; }
  delta[0] = delta[1] = delta[2] = 0.0;
  const double d0 = m00;
  if (!(d0 > 0)) return false;
  const double l10 = m01 / d0, l20 = m02 / d0;
  const double d1 = m11 - l10 * m01;
  if (!(d1 > 0)) return false;
  const double l21 = (m12 - l20 * m01) / d1;
  const double d2 = m22 - l20 * m02 - l21 * (l21 * d1);
  if (!(d2 > 0)) return false;
  const double y0 = r0, y1 = r1 - l10 * y0, y2 = r2 - l20 * y0 - l21 * y1;
  const double z2 = y2 / d2, z1 = y1 / d1 - l21 * z2, z0 = y0 / d0 - l10 * z1 - l20 * z2;
  delta[0] = z0; delta[1] = z1; delta[2] = z2;
  return true;
}

PAL_SOLVE_HD inline double quad_form(const double h6[6], const double s[3]) {
  return h6[0] * s[0] * s[0] + h6[3] * s[1] * s[1] + h6[5] * s[2] * s[2] + 2.0 * (h6[1] * s[0] * s[1] + h6[2] * s[0] * s[2] + h6[4] * s[1] * s[2]);
}

PAL_SOLVE_HD inline double clip(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// solve.lm_solve.  eval(x, sums) fills the sixteen sums at x (on the device: the whole workgroup calls it together and every lane
// receives the same values, so every lane takes the same path).  NS = kSumsLoss is solve.lm_solve_loss: the same iteration on
// the nineteen sums of a robust loss, the diagonal taken from sums [16..18].
template <int NS = kSums, class Eval>
PAL_SOLVE_HD inline void lm_solve(const double x0[3], const double lo[3], const double hi[3], int max_iter, Eval&& eval, double x[3], double* cost,
                            int* iters, int* stop_rule) {
  static_assert(NS == kSums || NS == kSumsLoss, "sixteen sums (linear) or nineteen (a robust loss)");
  double cur[NS], trial[NS], xn[3], s[3] = {0, 0, 0}, h6[6], delta[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) x[k] = clip(x0[k], lo[k], hi[k]);
  eval(x, cur);
  double lam = kLam0, nu = 2.0;
  int it = 0, stop = kStopNone;
  for (;;) {
    const double f = cur[15];
    const double diag[3] = {cur[NS == kSums ? 0 : 16], cur[NS == kSums ? 3 : 17], cur[NS == kSums ? 5 : 18]};
    bool held[3], flat = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double gk = cur[12 + k];
      held[k] = (x[k] <= lo[k] && gk > 0) || (x[k] >= hi[k] && gk < 0);
      flat = flat && (held[k] || fabs(gk) <= kGtol * sqrt(diag[k] * f));
    }
    if (flat) { stop = kStopGradient; break; }
    if (it >= max_iter) { stop = kStopCap; break; }
    ++it;
#pragma unroll
    for (int q = 0; q < 6; ++q) h6[q] = cur[q] + cur[6 + q];
    bool ok = damped_step(h6, diag, cur + 12, lam, held, delta);
    if (!ok) {
#pragma unroll
      for (int q = 0; q < 6; ++q) h6[q] = cur[q];
      ok = damped_step(h6, diag, cur + 12, lam, held, delta);
    }
    double fn = 0.0;
    if (ok) {
      double step = 0.0, xmax = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        xn[k] = clip(x[k] + delta[k], lo[k], hi[k]);
        s[k] = xn[k] - x[k];
        step = fmax(step, fabs(s[k]));
        xmax = fmax(xmax, fabs(x[k]));
      }
      if (step <= kXtol * (kXtol + xmax)) { stop = kStopStep; break; }
      eval(xn, trial);
      fn = trial[15];
    }
    if (ok && fn < f) {
      const double pred = -(2.0 * (cur[12] * s[0] + cur[13] * s[1] + cur[14] * s[2]) + quad_form(h6, s));
      const double rho = pred > 0 ? (f - fn) / pred : 1.0;
      const bool small = (f - fn) <= kFtol * f && lam <= 1.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) x[k] = xn[k];
#pragma unroll
      for (int q = 0; q < NS; ++q) cur[q] = trial[q];
      const double t = 2.0 * rho - 1.0;
      lam = fmax(lam * fmax(1.0 / 3.0, 1.0 - t * t * t), kLamMin);
      nu = 2.0;
      if (small) { stop = kStopDecrease; break; }
    } else {
      lam = lam * nu;
      nu = 2.0 * nu;
      if (lam > kLamMax) { stop = kStopDamping; break; }
    }
  }
  *cost = 0.5 * cur[15];
  *iters = it;
  *stop_rule = stop;
}

// np.percentile(.., 75) from the two order statistics around the virtual index 0.75 (P - 1) (NumPy's _lerp)
PAL_SOLVE_HD inline int64_t percentile75_rank(int64_t P, double* t) {
  const double h = 0.75 * double(P - 1);
  const double lo = floor(h);
  *t = h - lo;
  return int64_t(lo);
}
PAL_SOLVE_HD inline double percentile_lerp(double a, double b, double t) {
  const double d = b - a;
  if (d == 0) return a;
  return t < 0.5 ? a + d * t : b - d * (1 - t);
}

// utils.dynamic_bounds_extended from the microphone extents and the percentile
PAL_SOLVE_HD inline void box_from(const double mn[3], const double mx[3], double pct, double buffer, double lo[3], double hi[3]) {
  const double extra = pct > 1.0 ? pct : 1.0;      // max(np.percentile(..), 1.0)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = mn[k] - (buffer + extra);
    hi[k] = mx[k] + (buffer + extra);
  }
}

// start s >= 1 of the g x g x g grid (x slowest): the cell centre
PAL_SOLVE_HD inline void grid_start(int cell, int g, const double lo[3], const double hi[3], double x[3]) {
  const int idx[3] = {cell / (g * g), (cell / g) % g, cell % g};
#pragma unroll
  for (int k = 0; k < 3; ++k) x[k] = lo[k] + (double(idx[k]) + 0.5) * ((hi[k] - lo[k]) / double(g));
}

// ---- np.sum / np.mean of a contiguous float64 array: NumPy's pairwise summation, so that snr / mean(snr) equals
// utils.compute_weights bit for bit.  Blocks of at most 128 elements are summed with eight running sums; longer ranges
// split at n / 2 rounded down to a multiple of 8.  np_plan lists the blocks and the order of the additions as a post-order
// program: entry >= 0 = push the sum of block `entry`, -1 = add the two values on top of the stack.
constexpr int kNpBlock = 128;
constexpr int kNpMaxLeaves = 1024, kNpMaxProgram = 2 * kNpMaxLeaves;

template <class Get> PAL_SOLVE_HD inline double np_leaf_sum(Get&& a, int64_t off, int n) {   // n <= 128
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res += a(off + i);
    return res;
  }
  double r[8];
  for (int k = 0; k < 8; ++k) r[k] = a(off + k);
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int k = 0; k < 8; ++k) r[k] += a(off + i + k);
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a(off + i);
  return res;
}

// -> number of leaves (0 when the tables are too small); leaf_off / leaf_len [kNpMaxLeaves], program [kNpMaxProgram], *nprog entries
PAL_SOLVE_HD inline int np_plan(int64_t n, int32_t* leaf_off, int32_t* leaf_len, int32_t* program, int* nprog) {
  // explicit stack of (offset, length, state): state 0 = visit, 1 = emit the addition
  int32_t so[48], sl[48], ss[48];
  int sp = 0, leaves = 0, np_ = 0;
  so[0] = 0; sl[0] = int32_t(n); ss[0] = 0; sp = 1;
  while (sp > 0) {
    --sp;
    const int32_t off = so[sp], len = sl[sp], st = ss[sp];
    if (st == 1) { program[np_++] = -1; continue; }
    if (len <= kNpBlock) {
      if (leaves >= kNpMaxLeaves) return 0;
      leaf_off[leaves] = off; leaf_len[leaves] = len;
      program[np_++] = leaves++;
      continue;
    }
    int32_t n2 = len / 2;
    n2 -= n2 % 8;
    if (sp + 3 > 48 || np_ + 3 > kNpMaxProgram) return 0;
    so[sp] = off; sl[sp] = len; ss[sp] = 1; ++sp;                 // after both halves: add
    so[sp] = off + n2; sl[sp] = len - n2; ss[sp] = 0; ++sp;       // right half second
    so[sp] = off; sl[sp] = n2; ss[sp] = 0; ++sp;                  // left half first
  }
  *nprog = np_;
  return leaves;
}

PAL_SOLVE_HD inline double np_run_program(const int32_t* program, int nprog, const double* leaf_sum) {
  double st[48];
  int sp = 0;
  for (int k = 0; k < nprog; ++k) {
    if (program[k] >= 0) st[sp++] = leaf_sum[program[k]];
    else { st[sp - 2] = st[sp - 2] + st[sp - 1]; --sp; }
  }
  return sp > 0 ? st[0] : 0.0;
}

}  // namespace solve
}  // namespace pal
