// Host checks of csrc/pair_route.h: the route of a pair-pipeline call against a restatement of the rules as the chain of booleans
// Engine::pair_correlations once computed, exhaustively over the plan shapes of the GPU cases x switches x calls x parameters.
// Built and run by tests/test_host_pair_route.py (no GPU needed):
//   hipcc -O2 -I pyaudiolocalization_amd/csrc tests/host/test_pair_route.cpp -o /tmp/test_pair_route
#include <cstdio>
#include <vector>

#include "pair_route.h"
#include "plan_geometry.h"

using namespace pal;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// a plan's shape from its cut, with the row tile and the chunks of output indices that pfa_split gives it (plan_geometry.h)
static RouteIn split(int n1, int n2, bool r89 = false) {
  const TileChunks t = pfa_tile_chunks(n1, n2);
  RouteIn f{};
  f.n = f.nout = n1 * n2; f.split = true; f.n1 = n1; f.n2 = n2; f.nch = t.nch; f.lm = t.lm; f.r89 = r89;
  return f;
}
static RouteIn whole(int n, int nout) {
  RouteIn f{};
  f.n = n; f.nout = nout; f.nch = 1;
  return f;
}

static std::vector<RouteIn> shapes() {
  return {split(89, 991, true),    // L = 44100, Rader-89 columns
          split(89, 991, false),   // ... with PAL_R89=0
          split(25, 3529),         // two chunks
          split(47, 1877),         // three chunks
          split(67, 1321),
          split(23, 3835),         // strips, 8192-point row tiles
          split(7, 6857),          // C3: strips, 16384-point row tiles
          split(17, 5647),         // C2
          split(3, 8017),          // lm = 14, few rows
          split(103, 233),         // C5: five chunks, four blocks
          split(59, 407),          // the stream chain: seven blocks
          split(91, 971),          // five chunks, sixteen blocks
          split(127, 695),         // six chunks
          split(5, 255),           // N2 < 256
          whole(12013, 12013), whole(4999, 4999), whole(88200, 88200), whole(3999, 3999), whole(50001, 50001),
          whole(24000, 12000),     // fractional delay: fewer outputs than points
          // either side of every threshold of the rules (not all of them cuts the engine would choose)
          split(25, 682), split(25, 683),                              // eleven / twelve column blocks
          split(23, 2728), split(23, 2729),                            // ... of four strips
          split(89, 255, true), split(89, 256, true),                  // N2 >= 256
          split(1, 4099), split(1, 4093),                              // lm = 14 / 13 with one chunk
          whole(4095, 4095), whole(4096, 4096), whole(50000, 50000)};  // the window of k_rows_lean
}

static RouteIn with(RouteIn f, bool table, bool corr, bool multi, long long npairs, bool stored_only, int peaks, int method, double mult,
                    bool fin_cols, bool fuse_peaks, bool lean_store, bool rows_lean, long long rows_lean_min) {
  f.table = table; f.corr = corr; f.multi = multi; f.npairs = npairs; f.stored_only = stored_only;
  f.num_peaks = peaks; f.threshold_method = method; f.threshold_multiplier = mult;
  f.fin_cols = fin_cols; f.fuse_peaks = fuse_peaks; f.lean_store = lean_store; f.rows_lean = rows_lean; f.rows_lean_min = rows_lean_min;
  return f;
}

// ---- the rules, restated: the predicates that lived in pfa.hip and the booleans of pair_correlations / run_group ----
static int old_blocks(const RouteIn& f) { return (f.n2 + (f.nch <= 1 ? 4 : 1) * 62 - 1) / ((f.nch <= 1 ? 4 : 1) * 62); }
static bool old_nohist(const RouteIn& p) { return p.threshold_method > 0 || (p.threshold_multiplier >= 0 && p.threshold_multiplier <= 2.0); }
static bool old_can_fuse(const RouteIn& f, const RouteIn& s) { return s.fuse_peaks && f.split && f.nch >= 1 && f.nch <= 4 && f.n2 >= 3; }
static bool old_can_finish(const RouteIn& f, const RouteIn& p, const RouteIn& s) {
  bool cols_ok = f.r89 || (f.nch >= 2 && f.nch <= 4) || (f.nch <= 1 && f.lm <= 13);
  if (!f.r89 && old_blocks(f) < 12) cols_ok = false;
  return s.fin_cols && old_can_fuse(f, s) && p.num_peaks == 1 && f.n2 >= 256 && cols_ok;
}
static bool old_can_lean_store(const RouteIn& f, const RouteIn& p, const RouteIn& s) {
  return s.lean_store && s.fin_cols && s.fuse_peaks && f.split && f.nch >= 1 && f.nch <= 4 && old_blocks(f) >= 12 && p.num_peaks == 1 && old_nohist(p);
}
static bool old_rows_can_lean(const RouteIn& f, const RouteIn& p, const RouteIn& s) {
  return s.rows_lean && s.fin_cols && p.num_peaks == 1 && old_nohist(p) && f.nout == f.n && f.n >= 4096 && f.n <= 50000;
}

static PairRoute old_route(const RouteIn& in) {
  const RouteIn &f = in, &c = in, &p = in;
  RouteIn s = in;
  if (c.stored_only) s.fin_cols = false;                       // the repair pass ran with the engine's switch turned off
  const bool pfa = f.split, table = c.table;
  const bool fin = table && pfa && !c.corr && !c.multi && old_can_finish(f, p, s);
  const bool lean = !fin && pfa && table && !c.multi && old_can_lean_store(f, p, s);
  const bool rlean = !fin && !lean && table && !c.multi && c.npairs >= s.rows_lean_min && old_rows_can_lean(f, p, s) && !(pfa && old_can_fuse(f, s));
  const bool fused = pfa && table && old_can_fuse(f, s);
  PairRoute r;
  if (lean) r.transform = RouteTransform::kLeanStore;
  else if (fin) r.transform = RouteTransform::kFinish;
  else if (fused) r.transform = RouteTransform::kFused;
  else if (pfa) r.transform = RouteTransform::kPfa;
  else r.transform = RouteTransform::kFourStep;
  if (rlean) r.stats = RouteStats::kRowsLean;
  else if (table && !fused && !fin && !lean) r.stats = RouteStats::kThreeLaunches;
  else r.stats = table ? RouteStats::kPass : RouteStats::kNone;
  CHECK(!(rlean && (fused || fin || lean)), "the restated rules give k_rows_lean beside a pass with its own statistics");
  return r;
}

static void check_grid() {
  long long cases = 0, seen[5][4] = {};
  for (const RouteIn& shape : shapes())
    for (int sw = 0; sw < 16; ++sw)
      for (long long rmin : {200000ll, 1ll})                        // PAL_ROWS_LEAN_MIN: the default, and 1 as the tests set it
        for (int call = 0; call < 16; ++call)
          for (int peaks : {1, 3})
            for (int method : {0, 1})
              for (double mult : {-1.0, 1.0, 2.0, 4.2})
                for (long long npairs : {2016ll, 200000ll}) {
                  const RouteIn f = with(shape, (call & 1) != 0, (call & 2) != 0, (call & 4) != 0, npairs, (call & 8) != 0, peaks, method, mult,
                                         (sw & 1) != 0, (sw & 2) != 0, (sw & 4) != 0, (sw & 8) != 0, rmin);
                  const RouteIn &c = f, &s = f;
                  const PairRoute got = pair_route(f), want = old_route(f);
                  ++cases;
                  ++seen[int(got.transform)][int(got.stats)];
                  CHECK(got.transform == want.transform && got.stats == want.stats,
                        "%d = %d x %d (nch %d lm %d r89 %d nout %d) switches %d min %lld call %d peaks %d method %d mult %g pairs %lld: route %d/%d, rules %d/%d",
                        f.n, f.n1, f.n2, f.nch, f.lm, int(f.r89), f.nout, sw, s.rows_lean_min, call, peaks, method, mult, npairs,
                        int(got.transform), int(got.stats), int(want.transform), int(want.stats));
                  const bool flags = got.transform == RouteTransform::kFinish || got.transform == RouteTransform::kLeanStore || got.stats == RouteStats::kRowsLean;
                  CHECK(got.flags_pairs() == flags, "flags_pairs");
                  if (c.stored_only) CHECK(!flags, "a stored-rows-only call of %d = %d x %d takes a route that flags pairs (%d/%d)", f.n, f.n1, f.n2,
                                           int(got.transform), int(got.stats));
                  if (!c.table) CHECK(got.stats == RouteStats::kNone && !flags, "no table, but statistics %d", int(got.stats));
                  if (c.table) CHECK(got.stats != RouteStats::kNone, "a table, but no statistics");
                  if (!f.split) CHECK(got.transform == RouteTransform::kFourStep, "no split, but transform %d", int(got.transform));
                }
  printf("%lld cases\n", cases);
  // every route occurs in the grid
  CHECK(seen[int(RouteTransform::kFinish)][int(RouteStats::kPass)] > 0, "no finish route in the grid");
  CHECK(seen[int(RouteTransform::kLeanStore)][int(RouteStats::kPass)] > 0, "no lean-store route in the grid");
  CHECK(seen[int(RouteTransform::kFused)][int(RouteStats::kPass)] > 0, "no fused route in the grid");
  for (RouteTransform t : {RouteTransform::kPfa, RouteTransform::kFourStep})
    for (RouteStats st : {RouteStats::kNone, RouteStats::kRowsLean, RouteStats::kThreeLaunches})
      CHECK(seen[int(t)][int(st)] > 0, "transform %d with statistics %d never occurs in the grid", int(t), int(st));
}

static void check_blocks() {
  for (int nch = 0; nch <= 6; ++nch)
    for (int n2 = 1; n2 <= 8192; ++n2) {
      RouteIn f{};
      f.n2 = n2; f.nch = nch;
      CHECK(fin_blocks(n2, nch) == old_blocks(f), "fin_blocks(%d, %d)", n2, nch);
    }
  CHECK(fin_blocks(991, 4) == 16 && fin_blocks(3529, 2) == 57 && fin_blocks(1877, 3) == 31 && fin_blocks(1321, 3) == 22 && fin_blocks(3835, 1) == 16 &&
            fin_blocks(233, 5) == 4 && fin_blocks(407, 3) == 7,
        "column blocks of the known forms (tests/host/test_fin_scratch.cpp kForms)");
}

// the routes the GPU tests expect (their profile-entry assertions), by name
static void check_pins() {
  // (shape, corr, multi, pairs, stored_only, peaks) with a table, the median threshold x 1.0 and these switches
  struct Sw { bool fin_cols; long long rows_lean_min; };
  auto route = [](const RouteIn& shape, bool corr, bool multi, long long npairs, bool stored_only, int peaks, Sw sw) {
    return pair_route(with(shape, true, corr, multi, npairs, stored_only, peaks, 0, 1.0, sw.fin_cols, true, true, true, sw.rows_lean_min));
  };
  auto is = [](PairRoute r, RouteTransform t, RouteStats s) { return r.transform == t && r.stats == s; };
  const Sw def{true, 200000}, nofin{false, 200000}, min1{true, 1};
  const RouteIn l44100 = split(89, 991, true), c5 = split(103, 233);
  CHECK(is(route(l44100, false, false, 2016, false, 1, def), RouteTransform::kFinish, RouteStats::kPass), "44100 samples, one peak, no corr: not the finishing pass");
  CHECK(is(route(l44100, true, false, 2016, false, 1, def), RouteTransform::kLeanStore, RouteStats::kPass), "44100 samples, one peak, corr: not the lean store");
  CHECK(is(route(l44100, false, false, 2016, false, 1, nofin), RouteTransform::kFused, RouteStats::kPass), "PAL_FIN=0: not fused");
  CHECK(is(route(l44100, false, false, 2016, true, 1, def), RouteTransform::kFused, RouteStats::kPass), "stored rows only: not fused");
  CHECK(is(route(l44100, false, true, 2016, false, 3, def), RouteTransform::kFused, RouteStats::kPass), "three peaks: not fused");
  CHECK(is(route(c5, false, false, 2016, false, 1, min1), RouteTransform::kPfa, RouteStats::kRowsLean), "103 x 233 with rows_lean_min = 1: not plain + k_rows_lean");
  CHECK(is(route(c5, false, false, 2016, false, 1, def), RouteTransform::kPfa, RouteStats::kThreeLaunches), "103 x 233, 2016 pairs: not plain + three launches");
  CHECK(is(route(c5, false, false, 200000, false, 1, def), RouteTransform::kPfa, RouteStats::kRowsLean), "103 x 233, 200 000 pairs: not plain + k_rows_lean");
  CHECK(is(route(c5, false, false, 200000, true, 1, def), RouteTransform::kPfa, RouteStats::kThreeLaunches), "103 x 233, stored rows only: not plain + three launches");
  CHECK(is(route(split(59, 407), false, false, 40000, false, 1, def), RouteTransform::kFused, RouteStats::kPass), "59 x 407 (seven blocks): not fused");
  CHECK(is(route(whole(12013, 12013), false, false, 200000, false, 1, def), RouteTransform::kFourStep, RouteStats::kRowsLean), "n = 12013, 200 000 pairs: not four-step + k_rows_lean");
  CHECK(is(route(whole(88200, 88200), false, false, 200000, false, 1, def), RouteTransform::kFourStep, RouteStats::kThreeLaunches), "n = 88200: not four-step + three launches");
  CHECK(is(pair_route(with(whole(4999, 4999), false, true, false, 1, false, 1, 0, 1.0, true, true, true, true, 200000)), RouteTransform::kFourStep, RouteStats::kNone),
        "no table: statistics");
  CHECK(nohist(1, 4.2) && nohist(0, 0.0) && nohist(0, 2.0) && !nohist(0, 2.5) && !nohist(0, -1.0), "nohist");
}

int main() {
  check_grid();
  check_blocks();
  check_pins();
  if (failures) { printf("%d FAILURES\n", failures); return 1; }
  printf("ALL OK\n");
  return 0;
}
