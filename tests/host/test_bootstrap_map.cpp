// Host checks of csrc/bootstrap_map.h against the specification (pyaudiolocalization_amd/bootstrap.py).  The Python side
// (tests/test_host_bootstrap_map.py) writes one case per line,
//   L i j s mode block_size seed digest [index 0 .. index L-1, when L <= 64]
// where digest is the 64-bit FNV-1a hash of shuffle_indices(...) as little-endian 32-bit words.  This program evaluates ShuffleMap at
// t = 0 .. L-1, hashes it the same way and compares; short rows are compared element by element, so a failure names the sample.
// Without a fixture: the Feistel network and the cycle walk against their inverses.  Built with the host sanitizers (no GPU needed):
//   hipcc -O2 -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I pyaudiolocalization_amd/csrc
//         tests/host/test_bootstrap_map.cpp -o /tmp/test_bootstrap_map
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bootstrap_map.h"

using namespace pal::boot;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t fnv1a(uint64_t h, uint32_t word) {
  for (int b = 0; b < 4; ++b) h = (h ^ ((word >> (8 * b)) & 0xFFu)) * 0x100000001B3ull;
  return h;
}
constexpr uint64_t kFnvBasis = 0xCBF29CE484222325ull;

// ---- the network and the walk against their inverses: every point of the 4^h domain, every x < n ----
static void check_inverses() {
  const uint64_t keys[] = {0ull, 0x0123456789ABCDEFull, ~0ull};
  for (uint32_t n : {1u, 2u, 4u, 5u, 16u, 17u, 1024u, 1025u}) {
    const int h = half_bits(n);
    const uint32_t dom = 1u << (2 * h);
    CHECK(dom >= n && (h == 1 || (dom >> 2) < n), "n = %u: h = %d", n, h);
    for (uint64_t key : keys) {
      std::vector<char> hit(dom, 0), hit_n(n, 0);
      for (uint32_t x = 0; x < dom; ++x) {
        const uint32_t y = feistel(x, key, h);
        CHECK(y < dom && !hit[y < dom ? y : 0], "n = %u key %llx: feistel(%u) = %u repeats or leaves the domain", n, (unsigned long long)key, x, y);
        if (y < dom) hit[y] = 1;
        CHECK(feistel_inv(y, key, h) == x, "n = %u key %llx: feistel_inv(feistel(%u)) = %u", n, (unsigned long long)key, x, feistel_inv(y, key, h));
        CHECK(feistel(feistel_inv(x, key, h), key, h) == x, "n = %u key %llx: feistel(feistel_inv(%u))", n, (unsigned long long)key, x);
      }
      for (uint32_t x = 0; x < n; ++x) {
        const uint32_t y = walk(x, key, n, h);
        CHECK(y < n && !hit_n[y < n ? y : 0], "n = %u key %llx: walk(%u) = %u repeats or leaves [0, n)", n, (unsigned long long)key, x, y);
        if (y < n) hit_n[y] = 1;
        CHECK(walk_inv(y, key, n, h) == x, "n = %u key %llx: walk_inv(walk(%u)) = %u", n, (unsigned long long)key, x, walk_inv(y, key, n, h));
        CHECK(walk(walk_inv(x, key, n, h), key, n, h) == x, "n = %u key %llx: walk(walk_inv(%u))", n, (unsigned long long)key, x);
      }
    }
  }
}

// ---- ShuffleMap against the specification's cases ----
static void check_cases(const char* path) {
  FILE* fh = fopen(path, "r");
  CHECK(fh != nullptr, "cannot read %s", path);
  if (!fh) return;
  int L, i, j, mode, bs, cases = 0, listed = 0;
  long long s;
  unsigned long long seed, digest;
  while (fscanf(fh, "%d %d %d %lld %d %d %llu %llu", &L, &i, &j, &s, &mode, &bs, &seed, &digest) == 8) {
    ++cases;
    if (L < 1 || L > (1 << 20) || bs < 1 || mode < 0 || mode > 2) { CHECK(false, "case %d: L %d mode %d block_size %d", cases, L, mode, bs); break; }
    const ShuffleMap map(key_of(seed, i, j, s), mode, uint32_t(L), uint32_t(bs));
    std::vector<char> hit(size_t(L), 0);
    uint64_t h = kFnvBasis;
    bool bijection = true;
    for (int t = 0; t < L; ++t) {
      const uint32_t src = map(uint32_t(t));
      h = fnv1a(h, src);
      if (src >= uint32_t(L) || hit[src]) bijection = false;
      else hit[src] = 1;
      if (L <= 64) {
        long long want = -1;
        if (fscanf(fh, "%lld", &want) != 1) { CHECK(false, "case %d: the index list ends at sample %d", cases, t); break; }
        CHECK((long long)src == want, "L %d (i, j, s) = (%d, %d, %lld) mode %d block_size %d seed %llu: sample %d comes from %u, specification %lld", L, i, j, s, mode,
              bs, seed, t, src, want);
      }
    }
    listed += L <= 64;
    CHECK(bijection, "L %d (i, j, s) = (%d, %d, %lld) mode %d block_size %d seed %llu: not a permutation of 0..L-1", L, i, j, s, mode, bs, seed);
    CHECK(h == digest, "L %d (i, j, s) = (%d, %d, %lld) mode %d block_size %d seed %llu: digest %016llx, specification %016llx", L, i, j, s, mode, bs, seed,
          (unsigned long long)h, digest);
  }
  CHECK(feof(fh), "case %d of %s does not parse", cases + 1, path);
  fclose(fh);
  printf("%d cases, %d of them with their index list\n", cases, listed);
  CHECK(cases >= 900 && listed >= 300, "only %d cases (%d listed) in %s", cases, listed, path);
}

int main(int argc, char** argv) {
  check_inverses();
  if (argc > 1) check_cases(argv[1]);
  else CHECK(false, "usage: test_bootstrap_map <cases>");
  if (failures) { printf("%d FAILURES\n", failures); return 1; }
  printf("ALL OK\n");
  return 0;
}
