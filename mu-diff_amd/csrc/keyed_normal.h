// The keyed Gaussian draw shared by ensemble.hip, known_region.hip, kspace.hip and slab.hip (through keyed_rows.h, the row toolkit on top):
// counter-based Philox4x64-10 (Random123; the algorithm and word order of numpy.random.Philox) and Box-Muller in fp64.  One Philox block
// gives 4 consecutive elements of one row; include/mudiff_hip.h (mud_randn_keyed) has the counter layout.
#pragma once
#include "mud_common.h"

#define ES_KEY_HI 0x4D55444946460001ull

// ---- Philox4x64-10 ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void es_philox_round(uint64_t& c0, uint64_t& c1, uint64_t& c2, uint64_t& c3, uint64_t k0, uint64_t k1) {
  const uint64_t lo0 = 0xD2E7470EE14C6C93ull * c0, hi0 = __umul64hi(0xD2E7470EE14C6C93ull, c0);
  const uint64_t lo1 = 0xCA5A826395121157ull * c2, hi1 = __umul64hi(0xCA5A826395121157ull, c2);
  const uint64_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
  c0 = n0;
  c1 = lo1;
  c2 = n2;
  c3 = lo0;
}

__device__ __forceinline__ void es_philox(uint64_t& c0, uint64_t& c1, uint64_t& c2, uint64_t& c3, uint64_t k0, uint64_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B97F4A7C15ull;
      k1 += 0xBB67AE8584CAA73Bull;
    }
    es_philox_round(c0, c1, c2, c3, k0, k1);
  }
}

// Box-Muller on one word pair, all in fp64: u1 in (0, 1], u2 in [0, 1)
__device__ __forceinline__ void es_box_muller(uint64_t wa, uint64_t wb, float& a, float& b) {
  const double u1 = (double)((wa >> 11) + 1) * 0x1.0p-53;
  const double u2 = (double)(wb >> 11) * 0x1.0p-53;
  const double r = sqrt(-2.0 * log(u1));
  double s, c;
  sincos(6.283185307179586 * u2, &s, &c);
  a = (float)(r * c);
  b = (float)(r * s);
}

// the 4 normals of Philox block `block` of the row keyed (slice, sample): elements 4*block .. 4*block + 3; word2 = (step << 8) | kind
__device__ __forceinline__ f32x4 es_block_normals(uint64_t block, uint64_t slice, uint64_t sample, uint64_t seed, uint64_t word2) {
  uint64_t c0 = block, c1 = slice, c2 = (sample << 32) | word2, c3 = 0;
  es_philox(c0, c1, c2, c3, seed, ES_KEY_HI);
  f32x4 v;
  float a, b;
  es_box_muller(c0, c1, a, b);
  v[0] = a;
  v[1] = b;
  es_box_muller(c2, c3, a, b);
  v[2] = a;
  v[3] = b;
  return v;
}
