// What the row kernels of the sampler share (known_region.hip, kspace.hip, slab.hip, slab_kspace.hip, band.hip and the keyed draws of
// ensemble.hip): a thread owns a quad, 4 consecutive floats of one row = one Philox block of keyed_normal.h.  The helpers here only
// index, load, store and draw: none holds a contractible floating-point expression, so every product and sum stays in the kernels, under
// their own `#pragma clang fp contract(off)` (which would not reach into a helper).  The level clamp itself is mud_level_index
// (mud_common.h), shared with elementwise.hip.
#pragma once
#include <type_traits>
#include "keyed_normal.h"

// ---- quad I/O: VEC = one 16-byte (mask: 4-byte) access, the caller vouches for row_len % 4 == 0 and the alignment; else element by
// element, cut to the n <= 4 elements the row still has.  Elements past n read as 0 (mask: false) and are not written.
template <bool VEC>
__device__ __forceinline__ f32x4 quad_load(const float* p, int n) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if constexpr (VEC) {
    v = *reinterpret_cast<const f32x4*>(p);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < n) v[e] = p[e];
  }
  return v;
}

template <bool VEC>
__device__ __forceinline__ void quad_store(float* p, f32x4 v, int n) {
  if constexpr (VEC) {
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < n) p[e] = v[e];
  }
}

template <bool VEC>
__device__ __forceinline__ void quad_load_mask(const uint8_t* p, int n, bool (&m)[4]) {
  if constexpr (VEC) {
    const uchar4 mv = *reinterpret_cast<const uchar4*>(p);
    m[0] = mv.x != 0;
    m[1] = mv.y != 0;
    m[2] = mv.z != 0;
    m[3] = mv.w != 0;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = e < n && p[e] != 0;
  }
}

// ---- the mapping of a one-dimensional launch: thread tid -> quad b of row r, at element `base`, n of its 4 elements inside the row
struct row_quad {
  int64_t r, b, base;
  int n;
};

template <bool VEC>
__device__ __forceinline__ bool row_quad_of(int64_t tid, int rows, int64_t row_len, int64_t blocks_per_row, row_quad& q) {
  if (tid >= (int64_t)rows * blocks_per_row) return false;
  q.r = tid / blocks_per_row;
  q.b = tid - q.r * blocks_per_row;
  q.base = q.r * row_len + 4 * q.b;
  q.n = VEC ? 4 : (int)(row_len - 4 * q.b < 4 ? row_len - 4 * q.b : 4);
  return true;
}

// ---- a keyed draw at a noise level, as one kernel argument.  eta: `noise` if given, else the keyed normals of (keys[r], seed, word2);
// level of row r: tables at / st of ntab entries at clamp(t[r] + toff); clean: neither is used.  No pointer here aliases an output.
struct keyed_level {
  const float* noise;
  const int64_t* keys;
  uint64_t seed, word2;
  const int64_t* t;
  int toff;
  const float *at, *st;
  int ntab, clean;
};

// the eta of the quad at element `base` of row r, which is Philox block `block` of that row
template <bool VEC>
__device__ __forceinline__ f32x4 quad_eta(const keyed_level& d, int64_t r, uint64_t block, int64_t base, int n) {
  return d.noise ? quad_load<VEC>(d.noise + base, n) : es_block_normals(block, (uint64_t)d.keys[2 * r], (uint64_t)d.keys[2 * r + 1], d.seed, d.word2);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
#define MUD_TRY(call)                 \
  do {                                \
    const int rc__ = (call);          \
    if (rc__ != MUD_OK) return rc__;  \
  } while (0)

// The checks every entry with a keyed draw makes, in two parts because the entries check their own pointers in between and a refusal
// must not change: first the numbers, which give word2, ...
static inline int keyed_step_word2(const char* who, int step, int kind, uint64_t& word2) {
  MUD_REQUIRE(step >= 0 && step < (1 << 24), "%s: step must be in [0, 2^24), got %d", who, step);
  word2 = ((uint64_t)step << 8) | (uint64_t)kind;
  return MUD_OK;
}

static inline int keyed_level_word2(const char* who, int ntab, int kind, int step, uint64_t& word2) {
  MUD_REQUIRE(ntab > 0, "%s: ntab must be > 0, got %d", who, ntab);
  MUD_REQUIRE(kind >= 0 && kind <= 15, "%s: kind must be in [0, 15], got %d", who, kind);
  return keyed_step_word2(who, step, kind, word2);
}

// ... then the operands (`used`: the entry launches something that reads them)
static inline int keyed_level_operands(const char* who, bool used, const keyed_level& d) {
  MUD_REQUIRE(!used || d.clean || (d.t && d.at && d.st), "%s: null pointer (t, a_tab, s_tab)", who);
  MUD_REQUIRE(!used || d.clean || d.noise || d.keys, "%s: without injected noise the draw needs keys", who);
  return MUD_OK;
}

// f(std::true_type) or f(std::false_type): one launch line for both instances of a kernel template <bool VEC, ...>
template <class F>
static inline void vec_dispatch(bool vec, F&& f) {
  if (vec) f(std::true_type{});
  else f(std::false_type{});
}
#define VEC_OF(v) decltype(v)::value
