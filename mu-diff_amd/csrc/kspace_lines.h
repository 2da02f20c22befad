// The line transforms and the column pass of the k-space constraints (kspace.hip, slab_kspace.hip; DESIGN.md sections 5.26, 5.28): batches
// of L = 2^logL lines of S complex values in LDS, built from kspace_fft.h's butterflies.  One copy of each, so that every kernel that
// transforms a line gives the same bits.
#pragma once
#include "kspace_fft.h"
#include "mud_common.h"

#pragma clang fp contract(off)   // a * y, D - ay: each rounded once, as tests/kspace_ref.py states them

#define KS_THREADS 256
#define KS_MIN_S 16
#define KS_MAX_S 512
// lines per workgroup: 16 (a column tile then moves 128 contiguous bytes per row), 8 at S = 512.  The line pitch is S + 1 complex
// values: the column pass stores one column per line, lanes one line apart, and an odd pitch spreads them over the 64 banks where the
// power of two S would put them all on two.  LDS: (lines * (S + 1) + S/2) * 8 bytes <= 34 880, several workgroups per CU.
static inline int ks_log_lines(int S) { return S > 256 ? 3 : 4; }
static inline size_t ks_lds_bytes_of(int S, int logL) { return ((size_t)(1 << logL) * (S + 1) + S / 2) * sizeof(float2); }
static inline size_t ks_lds_bytes(int S) { return ks_lds_bytes_of(S, ks_log_lines(S)); }

static inline int ks_log2(int S) {       // log2 of a supported size, else -1
  if (S < KS_MIN_S || S > KS_MAX_S || (S & (S - 1))) return -1;
  int l = 0;
  while ((1 << l) < S) ++l;
  return l;
}

__device__ __forceinline__ void ks_twiddles(float2* tw, int S) {
  for (int m = threadIdx.x; m < S / 2; m += KS_THREADS) {
    double s, c;
    sincospi(2.0 * (double)m / (double)S, &s, &c);       // (the argument is exact: S is a power of two)
    tw[m] = make_float2((float)c, (float)-s);
  }
}

// L = 2^logL lines of pitch P at x, natural order in, bit-reversed order out.  Starts and ends with a barrier.
__device__ __forceinline__ void ks_lines_dif(float2* x, int P, int logL, int logS, const float2* tw, bool conj) {
  const int n4 = 1 << (logL + logS - 2), n2 = 1 << (logL + logS - 1);
  __syncthreads();
  for (int lq = logS - 2; lq >= 0; lq -= 2) {
    for (int i = threadIdx.x; i < n4; i += KS_THREADS) ks_dif4(x + (i >> (logS - 2)) * P, i & ((1 << (logS - 2)) - 1), lq, logS, tw, conj);
    __syncthreads();
  }
  if (logS & 1) {
    for (int i = threadIdx.x; i < n2; i += KS_THREADS) ks_bfly2(x + (i >> (logS - 1)) * P, i & ((1 << (logS - 1)) - 1));
    __syncthreads();
  }
}

// the transpose: bit-reversed order in, natural order out
__device__ __forceinline__ void ks_lines_dit(float2* x, int P, int logL, int logS, const float2* tw, bool conj) {
  const int n4 = 1 << (logL + logS - 2), n2 = 1 << (logL + logS - 1);
  __syncthreads();
  if (logS & 1) {
    for (int i = threadIdx.x; i < n2; i += KS_THREADS) ks_bfly2(x + (i >> (logS - 1)) * P, i & ((1 << (logS - 1)) - 1));
    __syncthreads();
  }
  for (int lq = logS & 1; lq <= logS - 2; lq += 2) {
    for (int i = threadIdx.x; i < n4; i += KS_THREADS) ks_dit4(x + (i >> (logS - 2)) * P, i & ((1 << (logS - 2)) - 1), lq, logS, tw, conj);
    __syncthreads();
  }
}

// whose noise level slice r of the column pass takes: its own row's (mud_kspace_constrain) ...
struct ks_level_own {
  __device__ __forceinline__ int64_t operator()(int64_t r) const { return r; }
};

// Column pass: workgroup b owns the columns c0 .. c0 + L - 1 of slice r, one column per LDS line, in place in `data`.
//  !CON: DIF with the sign of `inverse`, scaled by 1/S, stored in natural order;
//   CON: forward DIF, D = . / S, residual = mask ? D - a * y : 0 at position p = frequency bitrev(p), inverse DIT, . / S; a at the level
//        of the row level_row(r) of t.
template <bool CON, class LEVEL_ROW>
__global__ __launch_bounds__(KS_THREADS) void k_ks_cols(float2* data, const float2* __restrict__ y, const uint8_t* __restrict__ mask, int mask_rows,
                                                        const int64_t* __restrict__ t, int toff, const float* __restrict__ at, int ntab, int clean,
                                                        int logS, int logL, int inverse, LEVEL_ROW level_row) {
  extern __shared__ float2 ks_lds[];
  const int S = 1 << logS, P = S + 1, L = 1 << logL;
  float2* x = ks_lds;
  float2* tw = ks_lds + L * P;
  const int tiles = S >> logL;
  const int64_t r = blockIdx.x / tiles;
  const int c0 = (int)(blockIdx.x - r * tiles) << logL;
  const float inv_s = 1.0f / (float)S;
  float2* slice = data + (r << (2 * logS));
  ks_twiddles(tw, S);
  for (int i = threadIdx.x; i < L * S; i += KS_THREADS) {
    const int l = i & (L - 1), u = i >> logL;
    x[l * P + u] = slice[(u << logS) + c0 + l];
  }
  ks_lines_dif(x, P, logL, logS, tw, CON ? false : inverse != 0);
  if constexpr (CON) {
    float a = 1.0f;
    if (!clean) a = at[mud_level_index(t, level_row(r), toff, ntab)];
    const uint8_t* m = mask + (mask_rows == 1 ? 0 : (r << (2 * logS)));
    const float2* ys = y + (r << (2 * logS));
    for (int i = threadIdx.x; i < L * S; i += KS_THREADS) {
      const int l = i & (L - 1), p = i >> logL;
      const int at_uv = (ks_bitrev(p, logS) << logS) + c0 + l;
      float2 res = make_float2(0.f, 0.f);
      if (m[at_uv]) {
        const float2 D = x[l * P + p], yv = ys[at_uv];
        const float dr = D.x * inv_s, di = D.y * inv_s, ar = a * yv.x, ai = a * yv.y;
        res = make_float2(dr - ar, di - ai);
      }
      x[l * P + p] = res;
    }
    ks_lines_dit(x, P, logL, logS, tw, true);
  }
  for (int i = threadIdx.x; i < L * S; i += KS_THREADS) {
    const int l = i & (L - 1), u = i >> logL;
    const float2 v = x[l * P + (CON ? u : ks_bitrev(u, logS))];
    slice[(u << logS) + c0 + l] = make_float2(v.x * inv_s, v.y * inv_s);
  }
}
