// bootstrap_map.h - the counter-based shuffle generator of the device bootstrap (bootstrap.hip), in exact 64-bit integer
// arithmetic; pyaudiolocalization_amd/bootstrap.py restates it bit for bit (the specification).  Host and device code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pal_hip.h"

namespace pal {
namespace boot {

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
constexpr int kRounds = 8;            // bootstrap.ROUNDS
constexpr uint64_t kShiftRound = 255;  // the circular shift's round of the round function

__host__ __device__ inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__host__ __device__ inline uint64_t key_of(uint64_t seed, int32_t i, int32_t j, int64_t s) {
  uint64_t k = mix64(seed + kGolden);
  k = mix64(k ^ uint64_t(int64_t(i)));
  k = mix64(k ^ uint64_t(int64_t(j)));
  return mix64(k ^ uint64_t(s));
}

// smallest h with 4^h >= n (h >= 1): the Feistel halves
__host__ __device__ inline int half_bits(uint32_t n) {
  int h = 1;
  while ((uint64_t(1) << (2 * h)) < n) ++h;
  return h;
}

__host__ __device__ inline uint32_t feistel(uint32_t x, uint64_t key, int h) {
  const uint32_t mask = (1u << h) - 1u;
  uint32_t l = x >> h, r = x & mask;
#pragma unroll
  for (int k = 0; k < kRounds; ++k) {
    const uint32_t f = uint32_t(mix64(key ^ (uint64_t(r) + (uint64_t(k) << 32)))) & mask;
    const uint32_t t = l ^ f;
    l = r;
    r = t;
  }
  return (l << h) | r;
}

__host__ __device__ inline uint32_t feistel_inv(uint32_t x, uint64_t key, int h) {
  const uint32_t mask = (1u << h) - 1u;
  uint32_t l = x >> h, r = x & mask;
#pragma unroll
  for (int k = kRounds - 1; k >= 0; --k) {
    const uint32_t f = uint32_t(mix64(key ^ (uint64_t(l) + (uint64_t(k) << 32)))) & mask;
    const uint32_t t = r ^ f;
    r = l;
    l = t;
  }
  return (l << h) | r;
}

// keyed bijection of [0, n) and its inverse: cycle-walking through the Feistel network over 4^h points
__host__ __device__ inline uint32_t walk(uint32_t x, uint64_t key, uint32_t n, int h) {
  do x = feistel(x, key, h); while (x >= n);
  return x;
}

__host__ __device__ inline uint32_t walk_inv(uint32_t x, uint64_t key, uint32_t n, int h) {
  do x = feistel_inv(x, key, h); while (x >= n);
  return x;
}

}  // namespace boot
}  // namespace pal

namespace pal {
namespace boot {

// Output sample t of one shuffle comes from source sample map(t).  The per-shuffle quantities (the key, the Feistel width,
// where the short last block lands, the circular shift) are set up once; map(t) is the per-sample part.
struct ShuffleMap {
  uint64_t key;
  int mode, h = 1;
  uint32_t L, bs, nb = 0, qs = 0, last = 0, at = 0, shift = 0;
  __host__ __device__ ShuffleMap(uint64_t k, int m, uint32_t len, uint32_t block) : key(k), mode(m), L(len), bs(block) {
    if (mode == PAL_BOOT_PERMUTATION) {
      h = half_bits(L);
    } else if (mode == PAL_BOOT_BLOCK) {
      nb = uint32_t((uint64_t(L) + bs - 1) / bs);
      h = half_bits(nb);
      qs = walk_inv(nb - 1, key, nb, h);   // output position of the short last block
      last = L - (nb - 1) * bs;            // its length (1 .. bs)
      at = qs * bs;                        // ... and where it starts
    } else {
      shift = uint32_t(mix64(key ^ (kShiftRound << 32)) % uint64_t(L));
    }
  }
  __host__ __device__ uint32_t operator()(uint32_t t) const {
    if (mode == PAL_BOOT_PERMUTATION) return walk(t, key, L, h);
    if (mode == PAL_BOOT_BLOCK) {
      uint32_t q, off;
      if (t < at) { q = t / bs; off = t - q * bs; }
      else if (t < at + last) { q = qs; off = t - at; }
      else { const uint32_t u = t - at - last; q = qs + 1 + u / bs; off = u - (q - qs - 1) * bs; }
      return walk(q, key, nb, h) * bs + off;
    }
    return t >= shift ? t - shift : t + L - shift;
  }
};

}  // namespace boot
}  // namespace pal
