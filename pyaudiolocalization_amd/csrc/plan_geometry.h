// Geometry of a transform plan (Engine::get_plan): which convolution a sequence length gets, whether the PHAT inverse takes a
// prime-factor cut, and the host-side tables of that cut.  Host code only, no HIP headers and no device calls:
// tests/host/test_plan_geometry.cpp compiles it alone, pins the plans the GPU tests expect, checks the invariants of every
// frame length up to 2^20 and compares against a table recorded from the device (tests/golden/plan_table.json).
// The engine allocates, uploads and launches from what these functions return (bluestein.hip alloc_conv, pfa.hip build_pfa);
// the launch helpers of conv_kernels.h dispatch on ConvGeom.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace pal {

// The engine's switches that shape a plan, read when the engine is created.
struct PlanSwitches {
  bool allow_r3 = true;      // PAL_RADIX3=0 forces power-of-two convolution lengths
  bool four_reg = true;      // PAL_FOUR_REG=0 keeps the four-step route on its LDS-tile passes (no register-resident rows)
  bool allow_pfa = true;     // PAL_PFA=0 keeps the PHAT inverse on the four-step chirp convolution
  bool allow_big = true;     // PAL_PFA_BIG=0: no register-resident row tiles of the cut (N2 <= 2048 only)
  bool allow_rader = true;   // PAL_RADER=0 keeps the cut's row pass on the in-LDS chirp convolution
  bool allow_r89 = true;     // PAL_R89=0: dense 89-point column DFTs instead of Rader's 8 x 11 convolution (pfa_rader89.h)
};

// ------------------------------------------------------------------ four-step chirp convolution
// One circular convolution of m = m1 x 2^l2 points (conv_kernels.h): m1-point column transforms, 2^l2-point row transforms.
enum class ConvKind {
  kLds,     // columns of 2^l1 points in LDS (k_cols_*), rows in LDS (k_rows)
  kLds3,    // columns of 3 * 2^l1 points in LDS (k_cols3_*), rows in LDS
  kReg,     // columns of m1 points in the registers of one lane (k_colsreg_*), rows in registers (k_rowsreg)
  kReg2     // columns of m1 points shared by two neighbouring lanes (k_colsreg2_*), rows in registers
};

struct ConvGeom {
  ConvKind kind = ConvKind::kLds;
  int m1 = 0;        // points per column
  int l1 = 0;        // the LDS kinds: m1 = 2^l1 or 3 * 2^l1 (0 for the register kinds)
  int l2 = 0;        // log2 of the points per row
  size_t m = 0;      // points per transform
  bool reg() const { return kind == ConvKind::kReg || kind == ConvKind::kReg2; }
};

// Register-resident rows where the columns then fit one lane comfortably: rows of 4096 points with 12 ... 24-point columns, or
// rows of 8192 points with 12 ... 24-point columns (measured on C2 / C3 / C5 and at n = 88 203 with the prime-factor route off:
// +13 ... +19 % over the LDS-tile passes either way, the shorter rows ahead where both fit); 32- and 48-point columns need
// 250 registers in one lane, so two neighbouring lanes share them (rows of 8192 points: C4's 393 216 = 48 x 8192, +5 %).
// A column length only needs a DFT that fits one lane - 2^a, 3 * 2^a, or 2 x 9 / 10 / 11 (reg_fft.h reg_dft) - so the
// convolution length is the smallest m1 x 2^12 / 2^13 that holds the sequence, in steps of about 10 % instead of the
// 2^k / 3 * 2^k ladder (88 203 points: 22 x 8192 = 180 224 instead of 196 608).
// The chooser walks this table in order; PAL_SWITCH_REG (conv_kernels.h) lists the same entries as l2 * 100 + m1.
struct RegGeom { int l2, m1; ConvKind kind; };
constexpr RegGeom kRegGeoms[] = {
    {12, 12, ConvKind::kReg}, {12, 16, ConvKind::kReg}, {12, 18, ConvKind::kReg}, {12, 20, ConvKind::kReg}, {12, 22, ConvKind::kReg},
    {12, 24, ConvKind::kReg},
    {13, 12, ConvKind::kReg}, {13, 16, ConvKind::kReg}, {13, 18, ConvKind::kReg}, {13, 20, ConvKind::kReg}, {13, 22, ConvKind::kReg},
    {13, 24, ConvKind::kReg}, {13, 32, ConvKind::kReg2}, {13, 48, ConvKind::kReg2}};

inline int ceil_log2(size_t v) {
  int l = 0;
  while ((size_t(1) << l) < v) ++l;
  return l;
}

// Geometry for at least `needed` points: the smaller of 2^k and 3 * 2^k (k >= 12 for the latter, so that a transform is a whole
// number of 4096-point row tiles), or a register geometry that is no longer.  False: more than 2^22 points, unsupported.
inline bool conv_geometry(size_t needed, const PlanSwitches& sw, ConvGeom* out) {
  int lm = ceil_log2(needed);
  if (lm < 12) lm = 12;
  if (lm > 22) return false;
  ConvGeom c;
  c.kind = ConvKind::kLds;
  c.m = size_t(1) << lm;
  c.l2 = lm <= 19 ? (lm - 6 < 10 ? lm - 6 : 10) : 11;
  c.l1 = lm - c.l2;
  const int k3 = lm - 2;                                   // 3 * 2^(lm-2) = 0.75 * 2^lm
  if (sw.allow_r3 && k3 >= 12 && (size_t(3) << k3) >= needed) {
    int l2 = k3 - 4 < 10 ? k3 - 4 : 10;
    int l1 = k3 - l2;
    if (l1 > 8) { l2 = 11; l1 = k3 - l2; }
    if (l1 >= 4 && l1 <= 8) {
      c.kind = ConvKind::kLds3;
      c.m = size_t(3) << k3;
      c.l1 = l1;
      c.l2 = l2;
    }
  }
  c.m1 = (c.kind == ConvKind::kLds3 ? 3 : 1) << c.l1;
  if (sw.four_reg) {
    const RegGeom* best = nullptr;
    size_t best_m = 0;
    for (const RegGeom& g : kRegGeoms) {
      const size_t m = size_t(g.m1) << g.l2;
      if (m < needed || m > c.m) continue;                 // (never longer than the 2^k / 3 * 2^k choice)
      if (!best || m < best_m) { best = &g; best_m = m; }  // ties: the shorter rows (they come first in the table)
    }
    if (best) {
      c.kind = best->kind;
      c.m = best_m;
      c.m1 = best->m1;
      c.l1 = 0;
      c.l2 = best->l2;
    }
  }
  *out = c;
  return true;
}

// ------------------------------------------------------------------ prime-factor cut of the PHAT inverse
constexpr int kColChunk = 11;    // output indices per accumulator chunk of the column pass (pfa_sample.h kPfaTC)
constexpr int kColUnroll = 4;    // zero rows behind the column table's last step (pfa_sample.h kPfaUnr)
constexpr int kRaderPrime = 991, kRaderR1 = 11, kRaderR2 = 9, kRaderR3 = 10;   // the Rader row pass: 990 = 11 x 9 x 10 (pfa_rader.h)
constexpr int kRader89 = 89;     // the Rader column transform (pfa_rader89.h kR89)

inline long long inv_mod(long long a, long long m) {   // a^-1 mod m (gcd = 1), 0 when m == 1
  if (m == 1) return 0;
  long long g = m, x = 0, y = 1, aa = a % m;
  while (aa) {
    const long long q = g / aa;
    long long t = g - q * aa; g = aa; aa = t;
    t = x - q * y; x = y; y = t;
  }
  return g == 1 ? ((x % m) + m) % m : -1;
}

inline long long gcd_ll(long long a, long long b) { while (b) { long long t = a % b; a = b; b = t; } return a; }

// Row tiles of 2^lm >= 2 N2 - 1 points (lm >= 9) and accumulator chunks of kColChunk output indices of the (N1 - 1) / 2 column steps
struct TileChunks { int lm, nch; };
inline TileChunks pfa_tile_chunks(long long n1, long long n2) {
  int lm = 9;
  while ((1ll << lm) < 2 * n2 - 1) ++lm;
  const int h = int((n1 - 1) / 2);
  return {lm, h > 0 ? (h + kColChunk - 1) / kColChunk : 1};
}

// Cut n = n1 x n2 (coprime, both odd; pfa.hip): n1 = 0 means no cut, the four-step convolution does the inverse.
struct PfaSplit {
  int n1 = 0, n2 = 0;         // N1 <= 127 (dense column DFTs), N2 <= 8192
  int lm = 0;                 // log2 of the row tile: 9..12 in LDS (pfa_kernels.h), 13..14 register-resident (pfa_big.h)
  int u1 = 0;                 // N2^-1 mod N1
  long long u2 = 0;           // N1^-1 mod N2, made even: the chirp exp(i pi u2 j^2 / N2) is then periodic mod N2 and symmetric
  long long e1 = 0, e2 = 0;   // CRT idempotents: k = (e1 k1 + e2 k2) mod n
  int nch = 1;                // accumulator chunks of the column pass
  bool rader = false;         // the row pass is Rader's convolution of N2 - 1 points (pfa_rader.h)
  bool r89 = false;           // the column pass may use Rader's 8 x 11 convolution (pfa_rader89.h)
};

// Best coprime split by a time model fitted to this part (microseconds per packed transform inside a launch group of
// 240): a row tile of 2^lm points costs kTile[lm] - 0.005 / 0.011 / 0.026 for the LDS-resident tiles of
// 1024 / 2048 / 4096 points (two per workgroup), 0.050 / 0.145 for the register-resident tiles of 8192 / 16384 (pfa_big.h:
// the 16384-point tile runs one workgroup per CU) - and the column pass 1.15e-5 n for its
// traffic plus 4e-8 N1 n for the dense N1-point DFTs.  The four-step route: 1.6e-5 per point of its convolution for the
// first two passes, 2.2e-5 n for the last pass and the statistics launches, x 0.86 with register-resident rows.  A split that cannot take the fused column
// pass (more than four chunks of output indices: N1 > 89) must beat the four-step route by 15 %.
inline PfaSplit pfa_split(long long n, long long nout, const ConvGeom& inv, const PlanSwitches& sw) {
  PfaSplit f;
  if (!sw.allow_pfa || nout != n || n < 3 || (n & 1) == 0) return f;
  static const double kTile[15] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0.003, 0.005, 0.0113, 0.026, 0.050, 0.145};
  double best = -1;
  int bn1 = 0, bn2 = 0;
  TileChunks bt{0, 1};
  for (long long d = 1; d <= 127 && d <= n; d += 2) {
    if (n % d) continue;
    const long long r = n / d;
    if (r > (sw.allow_big ? 8192 : 2048) || gcd_ll(d, r) != 1) continue;
    const TileChunks t = pfa_tile_chunks(d, r);
    // (16384-point tiles run one workgroup per CU for 45 us each: with few rows per transform the rounds of workgroups and the
    //  per-group fixed costs weigh more than the model says - 24 051 = 3 x 8017 measured 1.41 M pairs/s against 1.84 M on the
    //  four-step route, 48 k-point lengths break even: profiles/r02_g_length_sweep_*.csv)
    if (t.lm == 14 && n < 40000) continue;
    double cost = double(d) * kTile[t.lm] + double(n) * (1.15e-5 + 4e-8 * double(d));
    if (t.nch > 4) cost *= 1.15;
    if (best < 0 || cost < best) { best = cost; bn1 = int(d); bn2 = int(r); bt = t; }
  }
  const double four_step = (1.6e-5 * double(inv.m) + 2.2e-5 * double(n)) * (inv.reg() ? 0.86 : 1.0);
  if (best < 0 || best > four_step) return f;                  // the four-step route is no worse
  // (short transforms are launch-bound, the model does not apply: there the split must also stay within 1.5 x the
  //  four-step route's points, round 1's rule)
  if (n < 16384 && size_t(((bn1 + 1) / 2) * (2ll << bt.lm)) > inv.m + inv.m / 2) return f;
  f.n1 = bn1; f.n2 = bn2; f.lm = bt.lm; f.nch = bt.nch;
  f.u1 = int(inv_mod(bn2, bn1));
  f.u2 = inv_mod(bn1, bn2);
  if (bn2 == 1) f.u2 = 0;
  f.e1 = (long long)bn2 * f.u1 % n;
  f.e2 = (long long)bn1 * f.u2 % n;
  if (f.u2 & 1) f.u2 += bn2;                   // even multiplier
  f.rader = sw.allow_rader && bn2 == kRaderPrime;              // 991 is prime and 990 = 11 x 9 x 10
  f.r89 = sw.allow_r89 && bn1 == kRader89 && f.nch == 4;
  return f;
}

// ------------------------------------------------------------------ host tables of a cut
// cos / sin of 2 pi j t / N1 in the column pass's chunked order, the argument reduced exactly (j t mod N1) before the
// long-double evaluation; kColUnroll zero rows behind the last step
inline std::vector<double> pfa_col_table(int n1, int nch) {
  const int h = (n1 - 1) / 2;
  std::vector<double> tab(size_t(h + kColUnroll) * nch * 2 * kColChunk, 0.0);
  const long double two_pi = 6.283185307179586476925286766559005768L;
  for (int j = 1; j <= h; ++j)
    for (int t = 1; t <= h; ++t) {
      const int ch = (t - 1) / kColChunk, tt = (t - 1) % kColChunk;
      const long double ang = two_pi * (long double)((long long)j * t % n1) / (long double)n1;
      double* row = &tab[(size_t(j - 1) * nch + ch) * 2 * kColChunk];
      row[tt] = double(cosl(ang));
      row[kColChunk + tt] = double(sinl(ang));
    }
  return tab;
}

// twiddle bookkeeping of the row pass's last stage, which starts with `last_lp` bits done (fft_core.h stage_tw_last(lm)): per
// row of Y the index multiplier u1 row mod N1 and its step between outputs of a last-stage butterfly (pfa_kernels.h)
struct RowStep { int mult, step; };
inline std::vector<RowStep> pfa_row_table(int n1, int u1, int last_lp) {
  const long long P = 1ll << last_lp;
  std::vector<RowStep> rt(size_t(n1), RowStep{0, 0});
  for (int row = 0; row < n1; ++row) {
    const long long uk = (long long)u1 * row % n1;
    rt[size_t(row)] = RowStep{int(uk), int(uk * P % n1)};
  }
  return rt;
}

// Rader tables of the prime p = 991 (pfa_rader.h): the generator's powers and the re-indexing into prime-factor positions
// `pos` (mixed_radix.h Axes<11, 9, 10>::pos) of the convolution index
struct RaderIndex {
  int g = 0;                        // smallest primitive root (0: none found), order p - 1 checked on its prime factors
  std::vector<int> gpow;            // g^s mod p, s < p - 1
  std::vector<int> qidx, ridx;      // per bin of the row: position of a[s] = x[g^-s] (bin 0: p - 1, last) / of X[g^s] = x[0] + C[s]
};
inline RaderIndex rader_index(int p, int (*pos)(int)) {
  RaderIndex r;
  const int L = p - 1;
  for (int c = 2; c < p && !r.g; ++c) {
    bool ok = true;
    for (int q : {2, 3, 5, 11}) {
      long long x = 1, b = c;
      for (int ex = L / q; ex; ex >>= 1, b = b * b % p)
        if (ex & 1) x = x * b % p;
      ok = ok && x != 1;
    }
    if (ok) r.g = c;
  }
  if (!r.g) return r;
  r.gpow.assign(L, 0);
  r.qidx.assign(p, 0);
  r.ridx.assign(p, 0);
  long long x = 1;
  for (int s = 0; s < L; ++s, x = x * r.g % p) r.gpow[s] = int(x);
  for (int s = 0; s < L; ++s) {
    r.ridx[r.gpow[s]] = pos(s);                                // X[g^s] = x[0] + C[s]
    r.qidx[r.gpow[(L - s) % L]] = pos(s);                      // a[s] = x[g^-s]
  }
  r.qidx[0] = L;                                               // the rows of SP keep this order, bin 0 last
  return r;
}

// 3-D spectra of the kernel sequences w^(g^s), w = exp(+/- 2 pi i u2 / p), at position k2 + R2 k3 + R2 R3 k1:
// sum_s b[s] exp(-2 pi i ((s mod R2) k2 / R2 + (s mod R3) k3 / R3 + (s mod R1) k1 / R1));
// inverse direction scaled by 1 / (L n) (the unnormalised inverse stages and numpy's 1 / n), forward direction (the
// conjugate sequence) by 1 / L
struct Cplx { double re, im; };
struct RaderSpectra { std::vector<Cplx> inv, fwd; };
inline RaderSpectra rader_spectra(int p, long long n, long long u2, const std::vector<int>& gpow) {
  constexpr int R1 = kRaderR1, R2 = kRaderR2, R3 = kRaderR3;
  const int L = p - 1;
  const long double two_pi = 6.283185307179586476925286766559005768L;
  std::vector<long double> br(L), bi(L);                       // kernel sequence b[s] = w^(g^s), w = exp(2 pi i u2 / N2)
  for (int s = 0; s < L; ++s) {
    const long double ang = two_pi * (long double)(u2 * gpow[s] % p) / (long double)p;
    br[s] = cosl(ang);
    bi[s] = sinl(ang);
  }
  std::vector<long double> cr(L), ci(L);                       // exp(-2 pi i m / L)
  for (int s = 0; s < L; ++s) {
    const long double ang = -two_pi * (long double)s / (long double)L;
    cr[s] = cosl(ang);
    ci[s] = sinl(ang);
  }
  RaderSpectra out;
  out.inv.resize(L);
  out.fwd.resize(L);
  const long double scale = 1.0L / ((long double)L * (long double)n);
  for (int k1 = 0; k1 < R1; ++k1)
    for (int k3 = 0; k3 < R3; ++k3)
      for (int k2 = 0; k2 < R2; ++k2) {
        long double ar = 0, ai = 0, fr = 0, fi = 0;
        for (int s = 0; s < L; ++s) {
          const int m = int(((long long)(s % R2) * k2 * (L / R2) + (long long)(s % R3) * k3 * (L / R3) + (long long)(s % R1) * k1 * (L / R1)) % L);
          ar += br[s] * cr[m] - bi[s] * ci[m];
          ai += br[s] * ci[m] + bi[s] * cr[m];
          fr += br[s] * cr[m] + bi[s] * ci[m];                 // (br - i bi)(cr + i ci)
          fi += br[s] * ci[m] - bi[s] * cr[m];
        }
        const size_t at = size_t(k2) + size_t(R2) * k3 + size_t(R2) * R3 * k1;
        out.inv[at] = Cplx{double(ar * scale), double(ai * scale)};
        out.fwd[at] = Cplx{double(fr / (long double)L), double(fi / (long double)L)};
      }
  return out;
}

}  // namespace pal
