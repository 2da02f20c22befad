// The butterflies of kspace.hip's line transforms, as host/device functions of one butterfly index so that a
// host program can run them one by one (scripts/check_kspace_butterflies.cpp).
//
// A line is S = 2^logS complex fp32 values.  tw[m] = exp(-2 pi i m / S) for m < S/2, each component correctly rounded from fp64;
// `conj` takes the conjugate (the inverse transform's sign).  Two flow graphs, each the other's transpose:
//   decimation in frequency (DIF): natural order in, bit-reversed order out (position p holds frequency bitrev(p));
//   decimation in time (DIT):      bit-reversed order in, natural order out.
// A forward DIF followed by an inverse DIT therefore needs no permutation in between: the column pass of mud_kspace_constrain.
// A radix-4 pass is two radix-2 layers (spans 2q and q) done in registers on the 4 values base + {0, q, 2q, 3q}: half the LDS traffic
// and barriers of radix 2, and the order stays a plain bit reversal.  The second twiddle of the upper layer is the first times -+i,
// a swap and a sign.  An odd logS leaves one radix-2 layer of span 1, whose twiddle is 1.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)      // every product and sum below rounds once: the same bits from every kernel that includes this

__host__ __device__ __forceinline__ float2 ks_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__host__ __device__ __forceinline__ float2 ks_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__host__ __device__ __forceinline__ float2 ks_mul(float2 a, float2 w) {
  const float rr = a.x * w.x, ii = a.y * w.y, ri = a.x * w.y, ir = a.y * w.x;
  return make_float2(rr - ii, ri + ir);
}
// a * (-i) forward, a * (+i) with conj
__host__ __device__ __forceinline__ float2 ks_rot(float2 a, bool conj) { return conj ? make_float2(-a.y, a.x) : make_float2(a.y, -a.x); }
__host__ __device__ __forceinline__ float2 ks_tw(const float2* tw, int m, bool conj) {
  const float2 w = tw[m];
  return conj ? make_float2(w.x, -w.y) : w;
}

// butterfly g in [0, S/4) of the DIF radix-4 pass with q = 2^lq (spans 2q, then q)
__host__ __device__ __forceinline__ void ks_dif4(float2* x, int g, int lq, int logS, const float2* tw, bool conj) {
  const int q = 1 << lq, j = g & (q - 1), base = ((g >> lq) << (lq + 2)) + j;
  const int m = j << (logS - 2 - lq);                       // j * S / (4q) < S/4
  const float2 w1 = ks_tw(tw, m, conj), w2 = ks_tw(tw, 2 * m, conj);
  const float2 x0 = x[base], x1 = x[base + q], x2 = x[base + 2 * q], x3 = x[base + 3 * q];
  const float2 a0 = ks_add(x0, x2), a2 = ks_mul(ks_sub(x0, x2), w1);
  const float2 a1 = ks_add(x1, x3), a3 = ks_mul(ks_rot(ks_sub(x1, x3), conj), w1);
  x[base] = ks_add(a0, a1);
  x[base + q] = ks_mul(ks_sub(a0, a1), w2);
  x[base + 2 * q] = ks_add(a2, a3);
  x[base + 3 * q] = ks_mul(ks_sub(a2, a3), w2);
}

// butterfly g in [0, S/4) of the DIT radix-4 pass with q = 2^lq (spans q, then 2q): ks_dif4's transpose
__host__ __device__ __forceinline__ void ks_dit4(float2* x, int g, int lq, int logS, const float2* tw, bool conj) {
  const int q = 1 << lq, j = g & (q - 1), base = ((g >> lq) << (lq + 2)) + j;
  const int m = j << (logS - 2 - lq);
  const float2 w1 = ks_tw(tw, m, conj), w2 = ks_tw(tw, 2 * m, conj);
  const float2 x0 = x[base], t1 = ks_mul(x[base + q], w2), x2 = x[base + 2 * q], t3 = ks_mul(x[base + 3 * q], w2);
  const float2 a0 = ks_add(x0, t1), a1 = ks_sub(x0, t1), a2 = ks_add(x2, t3), a3 = ks_sub(x2, t3);
  const float2 u2 = ks_mul(a2, w1), u3 = ks_rot(ks_mul(a3, w1), conj);
  x[base] = ks_add(a0, u2);
  x[base + q] = ks_add(a1, u3);
  x[base + 2 * q] = ks_sub(a0, u2);
  x[base + 3 * q] = ks_sub(a1, u3);
}

// butterfly g in [0, S/2) of the span-1 radix-2 layer (its own transpose; no twiddle)
__host__ __device__ __forceinline__ void ks_bfly2(float2* x, int g) {
  const float2 a = x[2 * g], b = x[2 * g + 1];
  x[2 * g] = ks_add(a, b);
  x[2 * g + 1] = ks_sub(a, b);
}

__host__ __device__ __forceinline__ int ks_bitrev(int v, int logS) { return (int)(__builtin_bitreverse32((unsigned)v) >> (32 - logS)); }
