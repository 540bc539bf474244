// Host checks of the SNR strip of the finishing column pass (csrc/pair_route.h: fin_strip, fin_strip_offset, fin_strip_window): its
// pieces for the lengths of the GPU tests and the metric run, that the column blocks' layout stores every sample of the strip exactly
// once and nothing else, and the finisher's containment rule.  Built and run by tests/test_host_fin_strip.py (no GPU needed), once
// more with -fsanitize=address,undefined:
//   hipcc -O2 -I pyaudiolocalization_amd/csrc tests/host/test_fin_strip.cpp -o /tmp/test_fin_strip
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pair_route.h"
#include "pfa_rader89.h"

using namespace pal;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

constexpr int kTC = 11;                      // output indices per chunk of the dense column DFT (pfa_kernels.h kPfaTC): 22 slots a wavefront

// the lag window of a call as Engine::fin_setup computes it (the reference's arithmetic on lag / fs), centre n2 - 1 = (n - 1) / 2
static void lag_window(int n, double fs, double med, int& win_lo, int& win_hi) {
  const int c = (n - 1) / 2;
  const double est = med * fs;
  long long k = est < double(n) ? (long long)est + 2 : (long long)n;
  while (k >= 0 && !(std::fabs(double(k) / fs) <= med)) --k;
  const long long lo = c - k, hi = c + k;
  win_lo = int(lo < 1 ? 1 : lo);
  win_hi = int(hi > n - 2 ? n - 2 : hi);
}
static int snr_half(int n) { const int w = int(0.01 * double(n)); return w > 1 ? w : 1; }

struct Shape { int n, n1, n2, nch; bool r89; double fs, med; };
// the three lengths of tests/test_gpu_fin_strip.py (Rader-89 columns, dense in two chunks, strips) and the metric run
static const Shape kShapes[] = {{22873, 89, 257, 4, true, 16000.0, 0.02}, {17075, 25, 683, 2, false, 16000.0, 0.02},
                                {16385, 5, 3277, 1, false, 16000.0, 0.02}, {88199, 89, 991, 4, true, 44100.0, 0.05}};

static void check_bounds() {
  for (const Shape& s : kShapes) {
    int lo, hi;
    lag_window(s.n, s.fs, s.med, lo, hi);
    const int w = snr_half(s.n), c = (s.n - 1) / 2, D = c - lo;
    const FinStrip st = fin_strip(s.n, true, lo, hi, w, true, true);
    CHECK(st.pieces == 3, "n %d: %d pieces", s.n, st.pieces);
    CHECK(st.lo[0] == 0 && st.hi[0] == D + w - 1, "n %d: low end [%d, %d]", s.n, st.lo[0], st.hi[0]);
    CHECK(st.lo[1] == lo - w && st.hi[1] == hi + w - 1, "n %d: centre [%d, %d]", s.n, st.lo[1], st.hi[1]);
    CHECK(st.lo[2] == s.n - D - w && st.hi[2] == s.n - 1, "n %d: high end [%d, %d]", s.n, st.lo[2], st.hi[2]);
    CHECK(st.base[0] == 0 && st.base[1] == D + w && st.base[2] == D + w + (hi - lo + 2 * w), "n %d: offsets %d %d %d", s.n, st.base[0], st.base[1], st.base[2]);
    CHECK(st.len == 2 * (D + w) + (hi - lo + 2 * w), "n %d: length %d", s.n, st.len);
    CHECK(double(st.len) <= kFinStripShare * s.n, "n %d: share", s.n);
    printf("n %d: window [%d, %d], snr_w %d, strip [%d, %d] [%d, %d] [%d, %d] = %d samples (%.1f %%)\n", s.n, lo, hi, w, st.lo[0], st.hi[0], st.lo[1],
           st.hi[1], st.lo[2], st.hi[2], st.len, 100.0 * st.len / s.n);
    // the centre piece alone is S = [win_lo - snr_w, win_hi + snr_w - 1]
    if (s.n == 88199) CHECK(st.hi[1] - st.lo[1] + 1 == 6172, "metric run: centre piece of %d samples", st.hi[1] - st.lo[1] + 1);
    // no strip: the call is not windowed, an empty window, the histogram body or stored rows, the switch, a window as wide as the row
    CHECK(!fin_strip(s.n, false, lo, hi, w, true, true).on(), "n %d: strip without a window", s.n);
    CHECK(!fin_strip(s.n, true, 1, 0, w, true, true).on(), "n %d: strip for an empty window", s.n);
    CHECK(!fin_strip(s.n, true, lo, hi, w, false, true).on(), "n %d: strip outside the per-wavefront finishing form", s.n);
    CHECK(!fin_strip(s.n, true, lo, hi, w, true, false).on(), "n %d: strip with the switch off", s.n);
    CHECK(!fin_strip(s.n, true, 1, s.n - 2, w, true, true).on(), "n %d: strip for a window as wide as the row", s.n);
    // windows clipped at either end of the row (their centre is not the row's): pieces inside the row, ascending, disjoint, and
    // the centre piece still holds the SNR window of every argmax inside the lag window
    const int wins[][2] = {{1, 400}, {s.n - 401, s.n - 2}, {1, 1}, {s.n - 2, s.n - 2}};
    for (const auto& wn : wins) {
      const FinStrip e = fin_strip(s.n, true, wn[0], wn[1], w, true, true);
      CHECK(e.on(), "n %d: no strip for the narrow clipped window [%d, %d]", s.n, wn[0], wn[1]);
      if (!e.on()) continue;
      int total = 0;
      for (int p = 0; p < e.pieces; ++p) {
        CHECK(e.lo[p] >= 0 && e.hi[p] <= s.n - 1 && e.lo[p] <= e.hi[p], "n %d window [%d, %d]: piece %d = [%d, %d]", s.n, wn[0], wn[1], p, e.lo[p], e.hi[p]);
        CHECK(p == 0 || e.lo[p] > e.hi[p - 1] + 1, "n %d window [%d, %d]: pieces %d and %d touch", s.n, wn[0], wn[1], p - 1, p);
        CHECK(e.base[p] == total, "n %d window [%d, %d]: offset of piece %d", s.n, wn[0], wn[1], p);
        total += e.hi[p] - e.lo[p] + 1;
      }
      for (int p = e.pieces; p < kFinStripPieces; ++p) CHECK(e.lo[p] > e.hi[p], "unused piece %d not empty", p);
      CHECK(total == e.len, "n %d window [%d, %d]: length", s.n, wn[0], wn[1]);
      for (int imax = wn[0]; imax <= wn[1]; ++imax) {
        int a, b;
        fin_snr_window(imax, w, s.n, a, b);
        if (fin_strip_window(e, a, b) < 0) { CHECK(false, "n %d window [%d, %d]: argmax %d inside the window is not held", s.n, wn[0], wn[1], imax); break; }
      }
    }
  }
}

// Every sample of the strip is stored by exactly one (block, wavefront, slot, lane) of the column blocks' layout, at its offset, and no
// other sample is stored: the enumeration of k_pfa_cols_fin's geometry (pfa_cols_fin.h) and fin_lean_r89's strip stores (pfa_fin_lean.h)
static void check_partition() {
  Rader89Tab tab;
  make_rader89_tab(tab);
  for (const Shape& s : kShapes) {
    int lo, hi;
    lag_window(s.n, s.fs, s.med, lo, hi);
    const FinStrip st = fin_strip(s.n, true, lo, hi, snr_half(s.n), true, true);
    const int N1 = s.n1, N2 = s.n2, h = (N1 - 1) / 2;
    const bool strips_mode = s.nch <= 1;
    const int nblk = fin_blocks(N2, s.nch), NW = strips_mode ? 4 : (s.nch == 2 ? 2 : (s.nch == 3 ? 3 : 4));
    const bool full = h == s.nch * kTC;
    std::vector<int> stored(size_t(st.len), 0);
    long long outside = 0, count = 0;
    for (int cb = 0; cb < nblk; ++cb)
      for (int wave = 0; wave < NW; ++wave) {
        const int ch = strips_mode ? 0 : wave;
        const int nstrips = strips_mode ? nblk * NW : nblk, strip = strips_mode ? cb * NW + wave : cb;
        const int c_lo = int((long long)strip * N2 / nstrips), c_hi = int((long long)(strip + 1) * N2 / nstrips);
        CHECK(c_hi - c_lo <= kColsOwn, "n %d: strip %d owns %d columns", s.n, strip, c_hi - c_lo);
        const bool active = strips_mode || ch < s.nch;
        // the slots' output indices and which of them exist (slot 0: t = 0)
        int slot_t[23];
        bool exists[23];
        slot_t[0] = 0;
        if (s.r89) {
          exists[0] = wave == 0;
          for (int i = 0; i < kR89Slots; ++i) { slot_t[1 + i] = tab.tmap[wave][i]; exists[1 + i] = true; }
        } else {
          exists[0] = active && ch == 0;
          for (int tt = 0; tt < kTC; ++tt) {
            const int tl = ch * kTC + tt + 1;
            slot_t[1 + tt] = tl;
            slot_t[1 + kTC + tt] = N1 - tl;
            exists[1 + tt] = exists[1 + kTC + tt] = active && (full || tl <= h);
          }
        }
        for (int slot = 0; slot < 23; ++slot) {
          if (!exists[slot]) continue;
          const int t = slot_t[slot];
          bool meets = false;                                   // slot_mask over the pieces' output indices
          for (int p = 0; p < st.pieces; ++p) meets = meets || (t >= st.lo[p] / N2 && t <= st.hi[p] / N2);
          for (int lane = 0; lane < 64; ++lane) {
            const int m2 = c_lo - 1 + lane;
            const bool live = m2 >= 0 && m2 < N2 && lane <= c_hi - c_lo + 1;
            const bool own = live && lane >= 1 && lane <= c_hi - c_lo;
            if (!own) continue;
            const int m = m2 + N2 * t;
            CHECK(m >= 0 && m < s.n, "n %d: sample %d", s.n, m);
            const int off = fin_strip_offset(st, m);
            if (off >= 0 && !meets) ++outside;                  // a sample of the strip in a slot the mask leaves out: never stored
            if (!meets || off < 0) continue;
            CHECK(off < st.len, "n %d: offset %d of sample %d beyond the strip (%d)", s.n, off, m, st.len);
            if (off < st.len) ++stored[size_t(off)];
            ++count;
          }
        }
      }
    int bad = 0;
    for (int v : stored) bad += v != 1;
    CHECK(bad == 0, "n %d: %d strip entries are not stored exactly once", s.n, bad);
    CHECK(outside == 0, "n %d: %lld samples of the strip sit in slots outside the mask", s.n, outside);
    CHECK(count == st.len, "n %d: %lld stores for %d entries", s.n, count, st.len);
    // offsets: ascending with the sample index, -1 exactly outside the pieces
    int next = 0;
    for (int m = 0; m < s.n; ++m) {
      bool in = false;
      for (int p = 0; p < st.pieces; ++p) in = in || (m >= st.lo[p] && m <= st.hi[p]);
      const int off = fin_strip_offset(st, m);
      if (in ? off != next : off != -1) { CHECK(false, "n %d: offset %d of sample %d", s.n, off, m); break; }
      next += in;
    }
  }
}

// The finisher sums the SNR window from the strip iff one piece holds all of it
static void check_containment() {
  for (const Shape& s : kShapes) {
    int lo, hi;
    lag_window(s.n, s.fs, s.med, lo, hi);
    const int w = snr_half(s.n), D = (s.n - 1) / 2 - lo;
    const FinStrip st = fin_strip(s.n, true, lo, hi, w, true, true);
    struct At { int imax; bool held; };
    const At at[] = {{lo, true}, {hi, true}, {lo - 1, false}, {hi + 1, false}, {0, true}, {s.n - 1, true}, {(lo + hi) / 2, true},
                     {D, true}, {D + 1, false}, {s.n - D, true}, {s.n - D - 1, false}, {w - 1, true}, {w, true}, {s.n - 1 - w, true}};
    for (const At& a : at) {
      int A, B;
      fin_snr_window(a.imax, w, s.n, A, B);
      CHECK(A >= 0 && B <= s.n && A < B, "n %d argmax %d: window [%d, %d)", s.n, a.imax, A, B);
      const int off = fin_strip_window(st, A, B);
      CHECK((off >= 0) == a.held, "n %d argmax %d: window [%d, %d) %s", s.n, a.imax, A, B, off >= 0 ? "held" : "not held");
      if (off >= 0) {                                           // consecutive entries of the strip, first to last sample
        CHECK(off == fin_strip_offset(st, A) && off + (B - A) - 1 == fin_strip_offset(st, B - 1), "n %d argmax %d: offsets", s.n, a.imax);
        CHECK(off + (B - A) <= st.len, "n %d argmax %d: the window ends beyond the strip", s.n, a.imax);
      }
    }
    // every argmax: held iff some piece holds the whole window (the rule restated), and a strip-less call holds nothing
    const FinStrip none = fin_no_strip();
    for (int imax = 0; imax < s.n; ++imax) {
      int A, B;
      fin_snr_window(imax, w, s.n, A, B);
      bool want = false;
      for (int p = 0; p < st.pieces; ++p) want = want || (A >= st.lo[p] && B - 1 <= st.hi[p]);
      if ((fin_strip_window(st, A, B) >= 0) != want || fin_strip_window(none, A, B) >= 0) { CHECK(false, "n %d argmax %d: rule", s.n, imax); break; }
    }
  }
}

int main() {
  check_bounds();
  check_partition();
  check_containment();
  if (failures) { printf("%d FAILURES\n", failures); return 1; }
  printf("ALL OK\n");
  return 0;
}
