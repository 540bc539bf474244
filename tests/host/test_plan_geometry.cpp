// Host checks of csrc/plan_geometry.h: the plans the GPU tests pin, the invariants of every frame length up to 2^20 under every
// plan switch, equality with a table recorded from the device (tests/golden/plan_table.json, flattened by the Python side into
// lines "<set> <L> n conv_len m1 m2 n1 n2 tile_len"), the Rader, row and column tables of the N1 x 991 family of
// tests/rader_family.py, and length -> plan -> pair_route() for the routes tests/test_gpu_peak_positions.py expects.  Built and run by tests/test_host_plan_geometry.py (no GPU needed):
//   hipcc -O2 -I pyaudiolocalization_amd/csrc tests/host/test_plan_geometry.cpp -o /tmp/test_plan_geometry
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fft_core.h"      // kPoints
#include "mixed_radix.h"   // Axes<11, 9, 10>::pos
#include "pair_route.h"
#include "plan_geometry.h"

using namespace pal;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// the plan of frames of L samples as Engine::get_plan(2 L - 1, L, 2 L - 1) builds it: the forward convolution (lin inputs, H
// outputs), the inverse one (n inputs, n outputs) and the cut
struct HostPlan { int n; bool ok; ConvGeom fwd, inv; PfaSplit cut; };
static HostPlan plan_of(int L, const PlanSwitches& sw) {
  HostPlan p{};
  p.n = 2 * L - 1;
  const int H = p.n / 2 + 1;
  p.ok = conv_geometry(size_t(L) + size_t(H) - 1, sw, &p.fwd) && conv_geometry(2 * size_t(p.n) - 1, sw, &p.inv);
  if (p.ok) p.cut = pfa_split(p.n, p.n, p.inv, sw);
  return p;
}
static int tile_len(const PfaSplit& f) { return f.n1 ? (f.rader ? f.n2 - 1 : 1 << f.lm) : 0; }   // as pal_plan_factors reports it

static PlanSwitches switches(const std::string& name) {
  PlanSwitches sw;
  if (name == "PAL_RADIX3=0") sw.allow_r3 = false;
  else if (name == "PAL_FOUR_REG=0") sw.four_reg = false;
  else if (name == "PAL_PFA_BIG=0") sw.allow_big = false;
  else if (name == "PAL_RADER=0") sw.allow_rader = false;
  else if (name == "PAL_PFA=0") sw.allow_pfa = false;
  else if (name == "PAL_R89=0") sw.allow_r89 = false;
  else CHECK(name == "default", "unknown switch set %s", name.c_str());
  return sw;
}
static const char* kSets[] = {"default", "PAL_RADIX3=0", "PAL_FOUR_REG=0", "PAL_PFA_BIG=0", "PAL_RADER=0", "PAL_PFA=0", "PAL_R89=0"};

// ---- (a) the values the GPU tests assert from the device ----
struct RaderCase { int n1, L, nch; };
static const RaderCase kRaderFamily[] = {{3, 1487, 1}, {9, 4460, 1}, {11, 5451, 1}, {23, 11397, 1}, {25, 12388, 2}, {45, 22298, 2}, {47, 23289, 3},
                                         {67, 33199, 3}, {69, 34190, 4}, {87, 43109, 4}, {91, 45091, 5}, {97, 48064, 5}, {113, 55992, 6},
                                         {127, 62929, 6}};

static void check_pins() {
  const PlanSwitches def;
  struct Cut { int L, n1, n2, tile; };   // tile 0: not pinned
  const Cut cuts[] = {{50, 1, 99, 512}, {496, 1, 991, 990}, {500, 1, 999, 2048}, {1000, 0, 0, 0}, {2500, 0, 0, 0}, {6007, 0, 0, 0},
                      {2048, 9, 455, 1024}, {2999, 3, 1999, 4096}, {3000, 7, 857, 0}, {5000, 11, 909, 0}, {10233, 5, 4093, 8192},
                      {24000, 7, 6857, 16384}, {12000, 103, 233, 512}, {11170, 89, 251, 0}, {44100, 89, 991, 990},
                      {11437, 89, 257, 0}, {8193, 5, 3277, 0}, {8538, 25, 683, 0}, {16051, 47, 683, 0}, {23564, 69, 683, 0}, {1008, 5, 403, 0},
                      {11962, 47, 509, 0}, {15525, 61, 509, 0}, {22651, 89, 509, 0}, {7890, 31, 509, 0}};
  for (const Cut& c : cuts) {
    const HostPlan p = plan_of(c.L, def);
    CHECK(p.ok && p.cut.n1 == c.n1 && p.cut.n2 == c.n2, "L = %d: cut %d x %d, pinned %d x %d", c.L, p.cut.n1, p.cut.n2, c.n1, c.n2);
    if (c.tile) CHECK(tile_len(p.cut) == c.tile, "L = %d: tile %d, pinned %d", c.L, tile_len(p.cut), c.tile);
    if (c.n1) CHECK((long long)c.n1 * c.n2 == p.n, "L = %d: %d x %d is not n", c.L, c.n1, c.n2);
  }
  // the Rader-row family (tests/rader_family.py): L = (991 N1 + 1) / 2, the smallest N1 of every class of the column passes
  for (const RaderCase& c : kRaderFamily) {
    const HostPlan p = plan_of(c.L, def);
    CHECK(2 * c.L - 1 == c.n1 * kRaderPrime, "L = %d is not (991 x %d + 1) / 2", c.L, c.n1);
    CHECK(p.ok && p.cut.n1 == c.n1 && p.cut.n2 == kRaderPrime && p.cut.rader && tile_len(p.cut) == kRaderPrime - 1 && p.cut.nch == c.nch,
          "L = %d: cut %d x %d, rader %d, tile %d, %d chunks; pinned %d x 991, %d chunks", c.L, p.cut.n1, p.cut.n2, int(p.cut.rader),
          tile_len(p.cut), p.cut.nch, c.n1, c.nch);
    CHECK(p.cut.r89 == false, "L = %d: Rader-89 columns", c.L);
  }
  {   // 92 163 = 93 x 991 = 31 x 2973: the model prefers the shorter columns, so a padded length between two of the family's is not a Rader plan
    const HostPlan p = plan_of(46082, def);
    CHECK(p.ok && p.cut.n1 == 31 && p.cut.n2 == 2973 && !p.cut.rader, "L = 46082: cut %d x %d, rader %d", p.cut.n1, p.cut.n2, int(p.cut.rader));
  }
  PlanSwitches norader;
  norader.allow_rader = false;
  CHECK(tile_len(plan_of(496, norader).cut) == 2048, "L = 496 with Rader off: tile %d", tile_len(plan_of(496, norader).cut));
  // the PHAT inverse's convolution with the prime-factor route off (test_gpu_parity.py REG_GEOMETRIES), and rows <= 2048 with the register route off
  PlanSwitches nopfa, lds;
  nopfa.allow_pfa = lds.allow_pfa = false;
  lds.four_reg = false;
  struct Reg { int L, m1, m2; };
  const Reg regs[] = {{12000, 12, 4096}, {16000, 16, 4096}, {18000, 18, 4096}, {20000, 20, 4096}, {22000, 22, 4096}, {24000, 24, 4096},
                      {30000, 16, 8192}, {36000, 18, 8192}, {40500, 20, 8192}, {44102, 22, 8192}, {48001, 24, 8192},
                      {60000, 32, 8192}, {90000, 48, 8192}};
  for (const Reg& r : regs) {
    const HostPlan p = plan_of(r.L, nopfa);
    CHECK(p.ok && p.inv.m1 == r.m1 && (1 << p.inv.l2) == r.m2 && p.cut.n1 == 0, "L = %d: %d x %d, pinned %d x %d", r.L, p.inv.m1, 1 << p.inv.l2, r.m1, r.m2);
    CHECK(p.inv.kind == (r.m1 > 24 ? ConvKind::kReg2 : ConvKind::kReg), "L = %d: kind %d", r.L, int(p.inv.kind));
    const HostPlan q = plan_of(r.L, lds);
    CHECK(q.ok && !q.inv.reg() && (1 << q.inv.l2) <= 2048, "L = %d with the register route off: rows of %d", r.L, 1 << q.inv.l2);
  }
  // frames above 98 304 samples (tests/long_frames.py RUNGS / CUTS): both ends of every rung of the LDS-tile convolutions and the five
  // long cuts; forward and inverse convolution under default switches and with the prime-factor route off, and the cut
  struct G3 { ConvKind kind; int a, l2; };   // a: l1 of the LDS kinds, m1 of the register kinds
  struct Long { int L; G3 inv, fwd; int n1, n2, lm, nch; };
  const ConvKind kL = ConvKind::kLds, k3 = ConvKind::kLds3, k2 = ConvKind::kReg2;
  const Long longs[] = {
      {98305, {kL, 9, 10}, {k2, 32, 13}, 0, 0, 0, 1},   {131072, {kL, 9, 10}, {k2, 32, 13}, 73, 3591, 13, 4},
      {131073, {k3, 8, 10}, {k2, 48, 13}, 65, 4033, 13, 3}, {196608, {k3, 8, 10}, {k2, 48, 13}, 0, 0, 0, 1},
      {196609, {kL, 9, 11}, {kL, 9, 10}, 0, 0, 0, 1},   {262144, {kL, 9, 11}, {kL, 9, 10}, 0, 0, 0, 1},
      {262145, {k3, 8, 11}, {k3, 8, 10}, 0, 0, 0, 1},   {393216, {k3, 8, 11}, {k3, 8, 10}, 0, 0, 0, 1},
      {393217, {kL, 10, 11}, {kL, 9, 11}, 0, 0, 0, 1},  {524288, {kL, 10, 11}, {kL, 9, 11}, 0, 0, 0, 1},
      {524289, {kL, 11, 11}, {k3, 8, 11}, 0, 0, 0, 1},  {786432, {kL, 11, 11}, {k3, 8, 11}, 0, 0, 0, 1},
      {786433, {kL, 11, 11}, {kL, 10, 11}, 0, 0, 0, 1}, {1048576, {kL, 11, 11}, {kL, 10, 11}, 0, 0, 0, 1},
      {131079, {k3, 8, 10}, {k2, 48, 13}, 119, 2203, 13, 6}, {196649, {kL, 9, 11}, {kL, 9, 10}, 93, 4229, 14, 5},
      {520129, {kL, 10, 11}, {kL, 9, 11}, 127, 8191, 14, 6}};
  const auto same = [](const ConvGeom& g, const G3& w) {
    const int m1 = w.kind == ConvKind::kLds ? 1 << w.a : (w.kind == ConvKind::kLds3 ? 3 << w.a : w.a);
    return g.kind == w.kind && g.m1 == m1 && g.l2 == w.l2 && g.l1 == (g.reg() ? 0 : w.a) && g.m == (size_t(m1) << w.l2);
  };
  for (const Long& c : longs) {
    const HostPlan p = plan_of(c.L, def), q = plan_of(c.L, nopfa);
    CHECK(p.ok && same(p.inv, c.inv) && same(p.fwd, c.fwd), "L = %d: inverse kind %d %d x 2^%d, forward kind %d %d x 2^%d", c.L, int(p.inv.kind),
          p.inv.m1, p.inv.l2, int(p.fwd.kind), p.fwd.m1, p.fwd.l2);
    CHECK(q.ok && same(q.inv, c.inv) && same(q.fwd, c.fwd) && q.cut.n1 == 0, "L = %d with the prime-factor route off: inverse kind %d %d x 2^%d, forward kind %d %d x 2^%d, cut %d",
          c.L, int(q.inv.kind), q.inv.m1, q.inv.l2, int(q.fwd.kind), q.fwd.m1, q.fwd.l2, q.cut.n1);
    CHECK(p.cut.n1 == c.n1 && p.cut.n2 == c.n2 && p.cut.lm == c.lm && p.cut.nch == c.nch && !p.cut.rader && !p.cut.r89, "L = %d: cut %d x %d, lm %d, %d chunks; pinned %d x %d, lm %d, %d chunks",
          c.L, p.cut.n1, p.cut.n2, p.cut.lm, p.cut.nch, c.n1, c.n2, c.lm, c.nch);
    if (c.n1) CHECK((long long)c.n1 * c.n2 == p.n && tile_len(p.cut) == (1 << c.lm) && (1 << c.lm) >= 2 * c.n2 - 1, "L = %d: %d x %d, tile %d", c.L, c.n1, c.n2, tile_len(p.cut));
  }
  {   // 520 129 is the longest frame that takes any cut, and its tile is the fullest (16 381 of 16 384 points)
    for (int L = 520130; L <= (1 << 20); ++L) CHECK(plan_of(L, def).cut.n1 == 0, "L = %d takes a cut", L);
    CHECK(2 * 8191 - 1 == 16381, "tile fill");
  }
  // pal_xcorr_vs_ref convolves 2 N - 1 points (tests/long_frames.py SPARSE_GEOM)
  struct X { int N; G3 g; };
  const X xs[] = {{196609, {kL, 9, 10}}, {262145, {k3, 8, 10}}, {393217, {kL, 9, 11}}, {524289, {k3, 8, 11}}, {1048576, {kL, 10, 11}}};
  for (const X& x : xs) {
    ConvGeom g;
    CHECK(conv_geometry(2 * size_t(x.N) - 1, def, &g) && same(g, x.g), "xcorr N = %d: kind %d %d x 2^%d", x.N, int(g.kind), g.m1, g.l2);
  }
}

// ---- (b) invariants ----
static void check_conv(const ConvGeom& g, size_t needed, int L) {
  CHECK(g.m >= needed, "L = %d: %zu points for %zu", L, g.m, needed);
  CHECK(g.m == (size_t(g.m1) << g.l2), "L = %d: m = %zu is not %d x 2^%d", L, g.m, g.m1, g.l2);
  bool ok = false;
  switch (g.kind) {   // what launch_cols_fwd / launch_rows / launch_cols_inv dispatch (conv_kernels.h), in whole tiles of their kernels
    case ConvKind::kLds:
      ok = g.l1 >= 6 && g.l1 <= 11 && g.l2 >= 6 && g.l2 <= 11 && g.m1 == (1 << g.l1) && g.m % kPoints == 0;
      break;
    case ConvKind::kLds3:   // columns in tiles of 3072 points (kPoints3), rows in tiles of kPoints
      ok = g.l1 >= 4 && g.l1 <= 8 && g.l2 >= 6 && g.l2 <= 11 && g.m1 == (3 << g.l1) && g.m % 3072 == 0 && g.m % kPoints == 0;
      break;
    case ConvKind::kReg:
    case ConvKind::kReg2:   // 256 (two lanes per column: 128) columns per workgroup (kRegCols)
      for (const RegGeom& r : kRegGeoms) ok = ok || (r.l2 == g.l2 && r.m1 == g.m1 && r.kind == g.kind);
      ok = ok && g.l1 == 0 && (1 << g.l2) % 256 == 0 && (g.kind == ConvKind::kReg2) == (g.m1 > 24);
      break;
  }
  CHECK(ok, "L = %d: kind %d, %d x 2^%d (l1 = %d) is nothing the launch switches accept", L, int(g.kind), g.m1, g.l2, g.l1);
}

static void check_invariants() {
  long long cuts = 0, kinds[4] = {};
  for (const char* set : kSets) {
    const PlanSwitches sw = switches(set);
    for (int L = 1; L <= (1 << 20); ++L) {
      const HostPlan p = plan_of(L, sw);
      CHECK(p.ok, "%s L = %d: no geometry", set, L);
      if (!p.ok) continue;
      check_conv(p.fwd, size_t(2 * L - 1), L);
      check_conv(p.inv, 2 * size_t(p.n) - 1, L);
      ++kinds[int(p.inv.kind)];
      if (!sw.four_reg) CHECK(!p.fwd.reg() && !p.inv.reg(), "%s L = %d: register rows", set, L);
      if (!sw.allow_r3) CHECK(p.fwd.kind != ConvKind::kLds3 && p.inv.kind != ConvKind::kLds3, "%s L = %d: radix 3", set, L);
      const PfaSplit& f = p.cut;
      if (!f.n1) continue;
      ++cuts;
      const long long n = p.n, n1 = f.n1, n2 = f.n2;
      CHECK(sw.allow_pfa, "%s L = %d: a cut", set, L);
      CHECK(n1 * n2 == n && (n1 & 1) && (n2 & 1) && gcd_ll(n1, n2) == 1 && n1 <= 127, "%s L = %d: cut %lld x %lld", set, L, n1, n2);
      CHECK(f.lm >= 9 && f.lm <= 14 && (1ll << f.lm) >= 2 * n2 - 1 && (f.lm == 9 || (1ll << (f.lm - 1)) < 2 * n2 - 1), "%s L = %d: %lld columns, lm = %d", set, L, n2, f.lm);
      CHECK(f.lm < 14 || n >= 40000, "%s L = %d: 16384-point tiles at n = %lld", set, L, n);
      if (!sw.allow_big) CHECK(f.lm <= 12, "%s L = %d: lm = %d", set, L, f.lm);
      CHECK(f.e1 >= 0 && f.e1 < n && (f.e1 - 1) % n1 == 0 && f.e1 % n2 == 0, "%s L = %d: e1 = %lld", set, L, f.e1);
      CHECK(f.e2 >= 0 && f.e2 < n && (f.e2 - 1) % n2 == 0 && f.e2 % n1 == 0, "%s L = %d: e2 = %lld", set, L, f.e2);
      CHECK((f.u1 * n2 - 1) % n1 == 0 && (f.u2 * n1 - 1) % n2 == 0 && (f.u2 & 1) == 0, "%s L = %d: u1 = %d, u2 = %lld", set, L, f.u1, f.u2);
      CHECK(f.nch == (n1 > 1 ? int(((n1 - 1) / 2 + 10) / 11) : 1), "%s L = %d: %d chunks for N1 = %lld", set, L, f.nch, n1);
      CHECK(f.rader == (sw.allow_rader && n2 == 991) && f.r89 == (sw.allow_r89 && n1 == 89), "%s L = %d: rader %d r89 %d", set, L, int(f.rader), int(f.r89));
    }
  }
  printf("%lld cuts; inverse convolutions by kind: %lld %lld %lld %lld\n", cuts, kinds[0], kinds[1], kinds[2], kinds[3]);
  for (int k = 0; k < 4; ++k) CHECK(kinds[k] > 0, "kind %d never chosen", k);
  ConvGeom g;
  CHECK(conv_geometry(size_t(1) << 22, PlanSwitches(), &g) && g.m == (size_t(1) << 22), "2^22 points");
  CHECK(!conv_geometry((size_t(1) << 22) + 1, PlanSwitches(), &g), "2^22 + 1 points are not refused");
  // the table's order decides ties: every entry is chosen for its own length (12 x 8192 apart: 24 x 4096 is as long and comes first)
  for (const RegGeom& r : kRegGeoms) {
    CHECK(conv_geometry(size_t(r.m1) << r.l2, PlanSwitches(), &g) && g.m == (size_t(r.m1) << r.l2), "%d x 2^%d", r.m1, r.l2);
    if (r.l2 == 12 || r.m1 > 12) CHECK(g.m1 == r.m1 && g.l2 == r.l2, "%d x 2^%d is never chosen", r.m1, r.l2);
  }
}

static void check_rader_tables() {
  using AX = Axes<kRaderR1, kRaderR2, kRaderR3>;
  const int p = kRaderPrime, L = p - 1;
  CHECK(AX::L == L, "axes");
  const RaderIndex ix = rader_index(p, [](int s) { return AX::pos(s); });
  CHECK(ix.g > 1 && int(ix.gpow.size()) == L && int(ix.qidx.size()) == p && int(ix.ridx.size()) == p, "generator %d", ix.g);
  if (failures) return;
  std::vector<int> seen(p, 0);
  long long x = 1;
  for (int s = 0; s < L; ++s, x = x * ix.g % p) {
    CHECK(ix.gpow[s] == int(x) && x >= 1 && !seen[x], "g^%d = %lld repeats: the order is not %d", s, x, L);
    seen[x] = 1;
  }
  CHECK(x == 1, "g^%d = %lld", L, x);
  std::vector<int> qs(p, 0), rs(L, 0);
  for (int s = 0; s < L; ++s) {
    CHECK(ix.ridx[ix.gpow[s]] == AX::pos(s), "ridx at g^%d", s);
    CHECK(ix.qidx[ix.gpow[(L - s) % L]] == AX::pos(s), "qidx at g^-%d", s);
  }
  for (int k = 0; k < p; ++k) {
    CHECK(ix.qidx[k] >= 0 && ix.qidx[k] < p && !qs[ix.qidx[k]]++, "qidx[%d] = %d", k, ix.qidx[k]);
    if (k) CHECK(ix.ridx[k] >= 0 && ix.ridx[k] < L && !rs[ix.ridx[k]]++, "ridx[%d] = %d", k, ix.ridx[k]);
  }
  CHECK(ix.qidx[0] == L, "qidx[0] = %d", ix.qidx[0]);
  // the kernel spectrum of a Rader convolution has unit-modulus bins apart from the first (|sum of all roots but 1| = 1): scaled 1 / (L n), 1 / L
  std::vector<int> family{89};
  for (const RaderCase& c : kRaderFamily) family.push_back(c.n1);
  for (int n1 : family) {
    const long long n = (long long)n1 * p, u2 = inv_mod(n1, p);
    CHECK(u2 > 0 && u2 < p && u2 * n1 % p == 1, "N1 = %d: u2 = %lld", n1, u2);
    const RaderSpectra sp = rader_spectra(p, n, u2, ix.gpow);
    CHECK(int(sp.inv.size()) == L && int(sp.fwd.size()) == L, "N1 = %d: spectra", n1);
    for (int k = 0; k < L && !failures; ++k) {
      const double want = k ? std::sqrt(double(p)) : 1.0;
      CHECK(std::fabs(std::hypot(sp.fwd[k].re, sp.fwd[k].im) * L - want) <= 1e-12 * want, "N1 = %d: forward bin %d", n1, k);
      CHECK(std::fabs(std::hypot(sp.inv[k].re, sp.inv[k].im) * L * double(n) - want) <= 1e-12 * want, "N1 = %d: inverse bin %d", n1, k);
      // position 0 is the plain sum of the sequence in both directions: all roots but 1, which is -1
      if (!k) CHECK(std::fabs(sp.fwd[0].re * L + 1.0) <= 1e-12 && std::fabs(sp.fwd[0].im * L) <= 1e-12 && std::fabs(sp.inv[0].re * L * double(n) + 1.0) <= 1e-12,
                    "N1 = %d: bin 0 is not -1", n1);
    }
    // what the engine hands over: the cut's u2 is made even (the chirp of the non-Rader tiles needs it), build_pfa() passes u2 mod N2
    const HostPlan hp = plan_of(int((n + 1) / 2), PlanSwitches());
    CHECK(hp.ok && hp.cut.n1 == n1 && (hp.cut.u2 & 1) == 0 && hp.cut.u2 % p == u2 && hp.cut.u2 < 2 * p, "N1 = %d: the cut's u2 = %lld, N1^-1 = %lld", n1, hp.cut.u2, u2);
    CHECK(hp.cut.u1 == int(inv_mod(p, n1)) && (long long)hp.cut.u1 * p % n1 == 1 % n1, "N1 = %d: u1 = %d", n1, hp.cut.u1);
    if (failures) return;
    // row table: per row k the twiddle index multiplier u1 k mod N1 and its step 2^last_lp times that
    for (int lp : {0, 7}) {
      const std::vector<RowStep> rows = pfa_row_table(n1, hp.cut.u1, lp);
      CHECK(int(rows.size()) == n1, "N1 = %d: %zu rows in the row table", n1, rows.size());
      for (int k = 0; k < n1 && k < int(rows.size()); ++k)
        CHECK(rows[k].mult == int((long long)hp.cut.u1 * k % n1) && rows[k].step == int(((long long)rows[k].mult << lp) % n1), "N1 = %d: row table at %d: %d, %d",
              n1, k, rows[k].mult, rows[k].step);
    }
    // column table [h + kColUnroll steps][nch chunks][cos x kColChunk | sin x kColChunk]: cos / sin(2 pi j t / N1) at step j, output index
    // t = chunk * kColChunk + tt + 1; zeros at every index beyond h (a last chunk that is not full) and in the kColUnroll rows behind step h
    // (k_pfa_fwd_cols and the inverse's column kernels run whole batches of kColUnroll steps)
    const int h = (n1 - 1) / 2, nch = hp.cut.nch;
    const std::vector<double> tab = pfa_col_table(n1, nch);
    CHECK(nch == (h + kColChunk - 1) / kColChunk && tab.size() == size_t(h + kColUnroll) * nch * 2 * kColChunk, "N1 = %d: column table of %zu entries", n1, tab.size());
    if (failures) return;
    for (int j = 1; j <= h + kColUnroll; ++j)
      for (int ch = 0; ch < nch; ++ch)
        for (int tt = 0; tt < kColChunk; ++tt) {
          const double* row = &tab[(size_t(j - 1) * nch + ch) * 2 * kColChunk];
          const int t = ch * kColChunk + tt + 1;
          if (j > h || t > h) CHECK(row[tt] == 0.0 && row[kColChunk + tt] == 0.0, "N1 = %d: column table at step %d, index %d is not zero", n1, j, t);
          else {
            const double ang = 6.283185307179586 * double((long long)j * t % n1) / double(n1);   // (two roundings of an angle below 2 pi: 1.4e-15)
            CHECK(std::fabs(row[tt] - std::cos(ang)) <= 4e-15 && std::fabs(row[kColChunk + tt] - std::sin(ang)) <= 4e-15, "N1 = %d: column table at step %d, index %d", n1, j, t);
          }
        }
  }
  // the column and row tables of 89 x 991
  const std::vector<double> T = pfa_col_table(89, 4);
  CHECK(T.size() == size_t(44 + kColUnroll) * 4 * 2 * kColChunk && std::fabs(T[0] - std::cos(6.283185307179586 / 89)) <= 1e-15 && T[T.size() - 1] == 0.0, "column table");
  const std::vector<RowStep> rt = pfa_row_table(89, 8, 7);
  CHECK(rt.size() == 89 && rt[1].mult == 8 && rt[1].step == 8 * 128 % 89 && rt[88].mult == 8 * 88 % 89, "row table");
}

// ---- (c) equality with the recorded table ----
static void check_table(const char* path) {
  FILE* fh = fopen(path, "r");
  CHECK(fh != nullptr, "cannot read %s", path);
  if (!fh) return;
  char set[64];
  int L, v[7], rows = 0;
  while (fscanf(fh, "%63s %d %d %d %d %d %d %d %d", set, &L, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]) == 9) {
    ++rows;
    const HostPlan p = plan_of(L, switches(set));
    const int got[7] = {p.n, int(p.inv.m), p.inv.m1, 1 << p.inv.l2, p.cut.n1, p.cut.n2, tile_len(p.cut)};
    CHECK(p.ok && !memcmp(got, v, sizeof got), "%s L = %d: n %d conv %d = %d x %d cut %d x %d tile %d; recorded n %d conv %d = %d x %d cut %d x %d tile %d", set, L,
          got[0], got[1], got[2], got[3], got[4], got[5], got[6], v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
  }
  fclose(fh);
  printf("%d recorded rows\n", rows);
  CHECK(rows >= 140, "only %d rows in %s", rows, path);
}

// ---- (d) length -> plan -> route, for the calls of tests/test_gpu_peak_positions.py (a table, one peak, at most 40 microphones) ----
static PairRoute route_of(int L, bool corr, double mult, int method, bool rows_lean, long long rows_lean_min) {
  const HostPlan p = plan_of(L, PlanSwitches());
  const PfaSplit& f = p.cut;
  return pair_route(RouteIn{p.n, p.n, f.n1 > 0, f.n1, f.n2, f.nch, f.lm, f.r89, true, corr, false, 780, false, 1, method, mult,
                            true, true, true, rows_lean, rows_lean_min});
}
static void check_routes() {
  struct Mode { int method; double mult; };
  const Mode modes[] = {{0, 1.0}, {1, 1.0}, {0, 4.2}};   // peak_positions.MODES: the last one needs histograms
  for (const Mode& m : modes) {
    const bool nh = nohist(m.method, m.mult);
    for (int L : {11437, 8193, 8538, 16051, 23564, 44100}) {                     // FIN
      const PairRoute r = route_of(L, false, m.mult, m.method, true, 200000);
      CHECK(r.transform == RouteTransform::kFinish && r.stats == RouteStats::kPass, "L = %d: not the finishing pass", L);
    }
    for (int L : {8193, 8538}) {                                                 // STORE: the caller wants the rows
      const PairRoute r = route_of(L, true, m.mult, m.method, true, 200000);
      CHECK(r.transform == (nh ? RouteTransform::kLeanStore : RouteTransform::kFused) && r.stats == RouteStats::kPass, "L = %d with rows: transform %d", L, int(r.transform));
    }
    for (int L : {1008, 11962}) {                                                // FUSED
      const PairRoute r = route_of(L, false, m.mult, m.method, true, 200000);
      CHECK(r.transform == RouteTransform::kFused && r.stats == RouteStats::kPass, "L = %d: not fused", L);
    }
    for (int L : {12000, 6007, 2500}) {                                          // ROWS_LEAN: PAL_ROWS_LEAN_MIN=1
      const PairRoute r = route_of(L, false, m.mult, m.method, true, 1);
      CHECK(r.transform == (L == 12000 ? RouteTransform::kPfa : RouteTransform::kFourStep) && r.stats == (nh ? RouteStats::kRowsLean : RouteStats::kThreeLaunches),
            "L = %d: %d / %d", L, int(r.transform), int(r.stats));
    }
    const PairRoute a = route_of(12000, false, m.mult, m.method, false, 200000), b = route_of(1000, false, m.mult, m.method, true, 200000);   // THREE
    CHECK(a.transform == RouteTransform::kPfa && a.stats == RouteStats::kThreeLaunches, "L = 12000, PAL_ROWS_LEAN=0: %d / %d", int(a.transform), int(a.stats));
    CHECK(b.transform == RouteTransform::kFourStep && b.stats == RouteStats::kThreeLaunches, "L = 1000: %d / %d", int(b.transform), int(b.stats));
  }
}

int main(int argc, char** argv) {
  check_pins();
  check_invariants();
  check_rader_tables();
  if (argc > 1) check_table(argv[1]);
  else CHECK(false, "usage: test_plan_geometry <flattened plan table>");
  check_routes();
  if (failures) { printf("%d FAILURES\n", failures); return 1; }
  printf("ALL OK\n");
  return 0;
}
