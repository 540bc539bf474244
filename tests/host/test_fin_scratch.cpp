// Host checks of csrc/fin_scratch.h: the layout of the finishing pass's per-stream scratch block and the rule that zeroes it.
// Built and run by tests/test_host_fin_scratch.py (no GPU needed):
//   hipcc -O2 -I pyaudiolocalization_amd/csrc tests/host/test_fin_scratch.cpp -o /tmp/test_fin_scratch
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fin_scratch.h"

using namespace pal;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// The forms of the finishing pass at 44.1 kHz (tests/test_gpu_parity.py FIN_CASES), from the plans' N1 x N2 (pal_plan_info /
// pal_plan_factors): nblk = ceil(N2 / 62) column blocks (kColsOwn), ceil(N2 / 248) for one-chunk strips (N1 <= 23); the grid has N1
// rows.  The last entry is the layout of a removed form (the four-step last pass at L = 44101: 34 blocks, 22 rows), kept as one more
// geometry for the reset rule.
struct Form { int L, nblk, grid_rows; };
static const Form kForms[] = {{44100, 16, 89},    // 89 x 991, Rader-89 columns
                              {44113, 57, 25},    // 25 x 3529
                              {44110, 31, 47},    // 47 x 1877
                              {44254, 22, 67},    // 67 x 1321
                              {44103, 16, 23},    // 23 x 3835, strips
                              {44101, 34, 22}};   // a 34-block, 22-row layout (once the four-step last pass)
static const int kGroups[] = {240, 32};           // the automatic group size at 44.1 kHz, and pal_set_chunk(32)

struct Geo { int L, gmax, nblk, grid_rows; FinLayout lay; };

static std::vector<Geo> geometries() {
  std::vector<Geo> g;
  for (const Form& f : kForms)
    for (int G : kGroups) g.push_back({f.L, G, f.nblk, f.grid_rows, fin_layout(G, f.nblk, f.grid_rows)});
  return g;
}

static size_t done_end(const Geo& g) { return size_t(g.gmax) * g.nblk * 6 * sizeof(unsigned); }

static void check_layouts(const std::vector<Geo>& geo) {
  for (const Geo& g : geo) {
    const FinLayout& l = g.lay;
    const size_t emax_end = l.off_emax + size_t(2 * g.gmax) * g.nblk * 12 * sizeof(double);
    const size_t parts_end = l.off_parts + size_t(2 * g.gmax) * g.nblk * 6 * kFinPartialBytes;
    const size_t edge_end = l.off_edge + size_t(2 * g.gmax) * 4 * g.grid_rows * sizeof(double);
    CHECK(l.off_emax % 128 == 0 && l.off_parts % 128 == 0 && l.off_edge % 128 == 0, "L %d G %d: regions not 128-byte aligned", g.L, g.gmax);
    CHECK(done_end(g) <= l.off_emax && emax_end <= l.off_parts && parts_end <= l.off_edge, "L %d G %d: regions overlap", g.L, g.gmax);
    CHECK(l.total >= edge_end, "L %d G %d: total %zu does not cover the edge region (%zu)", g.L, g.gmax, l.total, edge_end);
  }
}

// The hazard the rule guards against, on record: a layout B whose `done` words lie on bytes where a layout A kept maxima or partials,
// both inside one block (the block a mixed sequence leaves: the largest of them)
static void check_hazard_exists(const std::vector<Geo>& geo) {
  size_t block = 0;
  for (const Geo& g : geo) block = g.lay.total > block ? g.lay.total : block;
  int pairs = 0;
  for (const Geo& a : geo)
    for (const Geo& b : geo) {
      if (&a == &b || b.lay.total > block || a.lay.total > block) continue;
      if (done_end(b) > a.lay.off_emax) {            // B's done words reach into A's emax / parts (done_end(a) <= a.off_emax always)
        if (pairs < 4) printf("hazard: L %d G %d -> L %d G %d (done words up to %zu over emax from %zu)\n", a.L, a.gmax, b.L, b.gmax,
                              done_end(b), a.lay.off_emax);
        ++pairs;
      }
    }
  printf("%d ordered pairs of layouts share done / emax-or-parts bytes\n", pairs);
  CHECK(pairs >= 1, "no layout pair of the real geometries overlaps: the hazard is not on record");
}

static void check_predicate() {
  FinKey k;
  k.gmax = 240; k.nblk = 16; k.grid_rows = 89; k.block = 1 << 20;
  for (unsigned e : {0u, 1u, 2u, 1000u, kFinEpochWrap - 1}) CHECK(!fin_must_zero(k, k, e, kFinEpochWrap), "same key, epoch %u: zeroed", e);
  for (unsigned e : {kFinEpochWrap, kFinEpochWrap + 1}) CHECK(fin_must_zero(k, k, e, kFinEpochWrap), "same key, epoch %u: not zeroed at the wrap", e);
  CHECK(!fin_must_zero(k, k, 2, 3) && fin_must_zero(k, k, 3, 3), "wrap 3");
  for (int field = 0; field < 4; ++field)
    for (unsigned e : {0u, 1u, 7u}) {
      FinKey n = k;
      if (field == 0) n.gmax = 32;
      if (field == 1) n.nblk = 57;
      if (field == 2) n.grid_rows = 25;
      if (field == 3) n.block = 2 << 20;
      CHECK(fin_must_zero(k, n, e, kFinEpochWrap), "field %d changed, epoch %u: not zeroed", field, e);
    }
  CHECK(fin_must_zero(FinKey(), k, 0, kFinEpochWrap), "first launch of a slot: not zeroed");
}

// One stream slot driven through a sequence of layouts, 128-byte granules tagged with what their last writer kept there (`done`
// words or other entries) and its reset cycle.  A launch may trust its `done` words only if each granule under them is zero or
// held `done` words of the same cycle: then it holds an older epoch of this cycle, never the current one.
// `rule`: 0 = fin_must_zero and a whole-block reset, 1 = the earlier rule (zero only when the block grew or at the wrap, and then
// only the current layout's `total` bytes).
static int run_slot(const std::vector<Geo>& geo, const std::vector<int>& seq, unsigned wrap, int rule) {
  std::vector<long long> owner;                      // -1: zero; else 2 x cycle + 1 for done words, 2 x cycle for other entries
  size_t block = 0;
  FinKey prev;
  size_t prev_block = 0;
  unsigned epoch = 0;
  long long cycle = 0;
  int bad = 0;
  for (int idx : seq) {
    const Geo& g = geo[size_t(idx)];
    if (g.lay.total > block) {                       // Engine::scratch: a new block, zeroed
      block = g.lay.total;
      owner.assign((block + 127) / 128, -1);
    }
    FinKey key;
    key.gmax = g.gmax; key.nblk = g.nblk; key.grid_rows = g.grid_rows; key.block = block;
    bool zero;
    size_t zbytes;
    if (rule == 0) { zero = fin_must_zero(prev, key, epoch, wrap); zbytes = block; }
    else { zero = prev_block != block || epoch >= wrap; zbytes = g.lay.total; }
    if (zero) {
      for (size_t i = 0; i < (zbytes + 127) / 128; ++i) owner[i] = -1;
      epoch = 0;
      ++cycle;
      prev = key;
      prev_block = block;
    }
    ++epoch;
    const size_t nd = (done_end(g) + 127) / 128;
    for (size_t i = 0; i < nd; ++i)
      if (owner[i] != -1 && owner[i] != 2 * cycle + 1) { ++bad; break; }
    for (size_t i = 0; i < (g.lay.total + 127) / 128; ++i) owner[i] = 2 * cycle + (i < nd ? 1 : 0);
  }
  return bad;
}

static void check_sequences(const std::vector<Geo>& geo) {
  // every ordered pair of layouts, the largest first (so that no later one grows the block)
  const int m = int(geo.size());
  int big = 0;
  for (int i = 1; i < m; ++i) if (geo[size_t(i)].lay.total > geo[size_t(big)].lay.total) big = i;
  std::vector<int> pairs = {big};
  for (int a = 0; a < m; ++a)
    for (int b = 0; b < m; ++b)
      if (a != b) { pairs.push_back(a); pairs.push_back(b); }
  // one layout, then the others, across many wraps: small -> large and large -> small
  std::vector<int> wraps = {big};
  for (int r = 0; r < 7; ++r)
    for (int i = 0; i < m; ++i) for (int k = 0; k <= r % 4; ++k) wraps.push_back((i * 5 + r) % m);
  const int b0 = run_slot(geo, pairs, kFinEpochWrap, 0), b1 = run_slot(geo, wraps, 3, 0);
  CHECK(b0 == 0, "fin_must_zero: %d launches of the mixed sequence read done words over another layout's entries", b0);
  CHECK(b1 == 0, "fin_must_zero: %d launches across the wrap read done words of another layout or cycle", b1);
  // the earlier rule must fail both (this is what the model detects)
  const int p0 = run_slot(geo, pairs, kFinEpochWrap, 1), p1 = run_slot(geo, wraps, 3, 1);
  printf("earlier rule: %d stale launches in the mixed sequence, %d across the wrap\n", p0, p1);
  CHECK(p0 > 0 && p1 > 0, "the slot model no longer tells the earlier rule from fin_must_zero");
}

int main() {
  const std::vector<Geo> geo = geometries();
  check_layouts(geo);
  check_hazard_exists(geo);
  check_predicate();
  check_sequences(geo);
  if (failures) { printf("%d FAILURES\n", failures); return 1; }
  printf("ALL OK\n");
  return 0;
}
