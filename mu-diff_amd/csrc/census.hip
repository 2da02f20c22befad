// e4m3 range census of a convolution input (include/mudiff_hip.h: mud_e4m3_census) - the precision guard of MUD_PREC_FP8X.
//
// The plan converts every prologued activation a, and its fp16 remainder a - fp16(a), to e4m3 at CONSTANT power-of-two pre-scales
// (CM_X_SA, CM_X_SAL); its cross terms are only right while |a| stays inside about [5e-4, 112].  This kernel applies the staging
// arithmetic of the 3x3 convolution (conv_mfma.hip, cm_stage4: __builtin_fmaf(x, scale, shift), cm_fast_silu, the fp16 hi piece
// saturating at +-65504, the remainder a - hi; every piece of it from mud_common.h) to each element once and counts the elements
// whose images would saturate or flush.  It changes nothing: it is a read-only pass beside the convolution.
//
// Layout like GroupNorm pass 1 (groupnorm.hip): grid (pixel splits, B); a lane owns 4 channels (16 B per load; its 4 scales /
// shifts are read once) and walks a strided pixel range with CS_UNROLL loads in flight.  Counts are reduced per wave (shuffles)
// and per workgroup (LDS); then ONE integer atomic per counter per workgroup - integer sums and maxima do not depend on the order
// in which workgroups arrive, so the result is bit-reproducible.
#include "mud_common.h"

#define CS_THREADS 256
#define CS_PIX_PER_LANE 128     // pixels per lane (and column) of one workgroup: fewer, longer workgroups keep the atomics of the
                                // per-workgroup merge (all on one cache line) off the critical path - DESIGN.md section 5.4
#define CS_UNROLL 4

struct CsCount {
  unsigned n, over, under, f16, amax;
};

template <int PRO>
__device__ __forceinline__ void cs_count4(const f32x4& rw, const f32x4& sc, const f32x4& sh, CsCount& k) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float a = rw[e];
    if (PRO == MUD_PRO_AFFINE || PRO == MUD_PRO_AFFINE_SILU) {      // the conv's prologue (cm_stage4)
      a = __builtin_fmaf(a, sc[e], sh[e]);
      if (PRO == MUD_PRO_AFFINE_SILU) a = cm_fast_silu(a);
    }
    const float m = fabsf(a);
    const float lo = a - (float)(mud_h16)mud_sat_h16(a);          // the fp16 remainder, hi saturated like the conv's converter
    const float ms = m * (float)(1 << CM_X_SA);                     // |e4m3 image of a| before conversion
    k.over += (ms > 448.0f || fabsf(lo) * (float)(1 << CM_X_SAL) > 448.0f) ? 1u : 0u;
    k.under += (ms > 0.0f && ms < 0x1p-9f) ? 1u : 0u;
    k.f16 += m > 65504.0f ? 1u : 0u;
    k.amax = max(k.amax, __float_as_uint(m));                       // |a| >= 0: integer order = float order (NaN above inf)
  }
  k.n += 4;
}

__device__ __forceinline__ unsigned cs_wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned cs_wave_max(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor(v, o, 64));
  return v;
}

// cols = C / 4 lanes per pixel; rows = pixels walked side by side by one workgroup (cols <= CS_THREADS), or 1 with the lanes of a
// row looping over the columns (cols > CS_THREADS).  Workgroup (s, b) covers pixels [s*chunk, (s+1)*chunk) of sample b.
template <int PRO>
__global__ __launch_bounds__(CS_THREADS) void k_e4m3_census(mud_census_args a, int64_t chunk, int cols, int rows,
                                                            mud_census_out* __restrict__ out) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t HW = (int64_t)a.H * a.W;
  const int64_t p0 = (int64_t)blockIdx.x * chunk;
  const int64_t p1 = p0 + chunk < HW ? p0 + chunk : HW;
  CsCount k = {0u, 0u, 0u, 0u, 0u};
  const bool wide = cols > CS_THREADS;
  const int row = wide ? 0 : tid / cols;
  if (row < rows) {
    for (int col = wide ? tid : tid % cols; col < cols; col += CS_THREADS) {
      f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
      if (PRO == MUD_PRO_AFFINE || PRO == MUD_PRO_AFFINE_SILU) {
        sc = *(const f32x4*)(a.pro_scale + (int64_t)b * a.pro_ld + 4 * col);
        sh = *(const f32x4*)(a.pro_shift + (int64_t)b * a.pro_ld + 4 * col);
      }
      const float* base = a.x + (int64_t)b * HW * a.ldx + 4 * col;
      for (int64_t p = p0 + row; p < p1; p += (int64_t)CS_UNROLL * rows) {
        f32x4 v[CS_UNROLL];
#pragma unroll
        for (int u = 0; u < CS_UNROLL; ++u)      // all loads first: CS_UNROLL x 16 B in flight per lane
          if (p + u * rows < p1) v[u] = *(const f32x4*)(base + (p + u * rows) * a.ldx);
#pragma unroll
        for (int u = 0; u < CS_UNROLL; ++u)
          if (p + u * rows < p1) cs_count4<PRO>(v[u], sc, sh, k);
      }
    }
  }
  __shared__ unsigned s_red[CS_THREADS / 64][5];
  const unsigned r[5] = {cs_wave_sum(k.n), cs_wave_sum(k.over), cs_wave_sum(k.under), cs_wave_sum(k.f16), cs_wave_max(k.amax)};
  if ((tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < 5; ++j) s_red[tid >> 6][j] = r[j];
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long t[4] = {0ull, 0ull, 0ull, 0ull};
    unsigned mx = 0u;
#pragma unroll
    for (int w = 0; w < CS_THREADS / 64; ++w) {
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] += s_red[w][j];
      mx = max(mx, s_red[w][4]);
    }
    unsigned long long* o = (unsigned long long*)out;            // n, n_over, n_under, n_fp16_over, amax_bits
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (t[j]) atomicAdd(o + j, t[j]);
    if (mx) atomicMax(o + 4, (unsigned long long)mx);
  }
}

extern "C" int mud_e4m3_census(const mud_census_args* ap, mud_census_out* out, void* stream) {
  MUD_REQUIRE(ap != nullptr && out != nullptr, "mud_e4m3_census: null argument struct or output");
  const mud_census_args a = *ap;
  MUD_REQUIRE(a.x != nullptr, "mud_e4m3_census: x is NULL");
  MUD_REQUIRE(a.B >= 1 && a.B <= 65535 && a.H >= 1 && a.W >= 1 && a.C >= 4 && a.C % 4 == 0,
              "mud_e4m3_census: need 1 <= B <= 65535, H, W >= 1 and C a positive multiple of 4 (got B=%d H=%d W=%d C=%d)", a.B, a.H, a.W, a.C);
  MUD_REQUIRE(a.ldx >= a.C && a.ldx % 4 == 0, "mud_e4m3_census: need ldx >= C and ldx %% 4 == 0 (got ldx=%d C=%d)", a.ldx, a.C);
  MUD_REQUIRE(mud_aligned16(a.x) && (((uintptr_t)out) & 7u) == 0, "mud_e4m3_census: x must be 16-byte and out 8-byte aligned");
  MUD_REQUIRE(a.pro_mode == MUD_PRO_NONE || a.pro_mode == MUD_PRO_AFFINE || a.pro_mode == MUD_PRO_AFFINE_SILU,
              "mud_e4m3_census: pro_mode must be MUD_PRO_NONE, MUD_PRO_AFFINE or MUD_PRO_AFFINE_SILU (got %d)", a.pro_mode);
  if (a.pro_mode != MUD_PRO_NONE)
    MUD_REQUIRE(a.pro_scale != nullptr && a.pro_shift != nullptr && mud_aligned16(a.pro_scale) && mud_aligned16(a.pro_shift) &&
                    a.pro_ld >= a.C && a.pro_ld % 4 == 0,
                "mud_e4m3_census: an affine prologue needs 16-byte aligned pro_scale / pro_shift rows with pro_ld >= C, pro_ld %% 4 == 0 (got pro_ld=%d)",
                a.pro_ld);
  const int64_t HW = (int64_t)a.H * a.W;
  const int cols = a.C / 4;
  MUD_REQUIRE(a.B * HW * cols < ((int64_t)1 << 31), "mud_e4m3_census: more than 2^31 float4 items (B*H*W*C/4)");
  const int rows = cols >= CS_THREADS ? 1 : CS_THREADS / cols;
  int64_t chunk = (int64_t)rows * CS_PIX_PER_LANE;
  if (mud_cdiv(HW, chunk) > 65535) chunk = mud_cdiv(HW, 65535);
  const dim3 grid((unsigned)mud_cdiv(HW, chunk), (unsigned)a.B);
  hipStream_t s = (hipStream_t)stream;
  if (a.pro_mode == MUD_PRO_NONE) hipLaunchKernelGGL(k_e4m3_census<MUD_PRO_NONE>, grid, dim3(CS_THREADS), 0, s, a, chunk, cols, rows, out);
  else if (a.pro_mode == MUD_PRO_AFFINE) hipLaunchKernelGGL(k_e4m3_census<MUD_PRO_AFFINE>, grid, dim3(CS_THREADS), 0, s, a, chunk, cols, rows, out);
  else hipLaunchKernelGGL(k_e4m3_census<MUD_PRO_AFFINE_SILU>, grid, dim3(CS_THREADS), 0, s, a, chunk, cols, rows, out);
  MUD_CHECK_LAUNCH("mud_e4m3_census");
  return MUD_OK;
}
