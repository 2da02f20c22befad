// On-device evaluation metrics of the test driver (include/mudiff_hip.h: mud_value_range, mud_quantize_u8, mud_slice_metrics_u8).
//
// The reference ends an evaluation in host numpy: the global min / max over every predicted and target slice, 8-bit quantisation
// with that range (engine/test.py:371-387), then PSNR / SSIM / MAE on the quantised images (tools/metric_calc.py:28-53).  These
// kernels do the same on the GPU, exactly:
//  - min / max do not depend on reduction order: per-workgroup reductions merged with integer atomics on an order-preserving
//    encoding of the fp32 bits; a NaN anywhere is reported as NaN (np.min semantics);
//  - the quantisation is numpy's fp32 expression operation for operation (IEEE subtract, divide, multiply, each rounded once,
//    no contraction), then clip and truncation: bit-identical to the host;
//  - every 7x7 window statistic of an 8-bit image is an integer (sum q <= 49*255, sum q*r <= 49*255^2 < 2^31), so the SSIM's
//    means, variances and covariance are exact and only the per-pixel formula (fp64) and the per-slice sum round.  The sum is a
//    fixed-order reduction (per-workgroup partials, then one pass in partial order), with no float atomics: the result is
//    bit-identical run to run and does not depend on how slices are batched.
#include "mud_common.h"

#define MR_THREADS 256
#define MR_MAX_BLOCKS 2048

// order-preserving uint32 encoding of fp32: a < b (as floats, -0 < +0) <=> enc(a) < enc(b)
__device__ __forceinline__ unsigned mr_enc(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mr_dec(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }

// ws: [0] enc(min), [1] enc(max), [2] NaN seen
__global__ void k_range_init(unsigned* __restrict__ ws) {
  ws[0] = mr_enc(__builtin_inff());
  ws[1] = mr_enc(-__builtin_inff());
  ws[2] = 0u;
}

__device__ __forceinline__ void mr_scan(const float* __restrict__ p, int64_t n, float& mn, float& mx, bool& nan) {
  const int64_t stride = (int64_t)gridDim.x * MR_THREADS;
  const int64_t t0 = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  int64_t done = 0;
  if ((((uintptr_t)p) & 15u) == 0) {
    const int64_t n4 = n / 4;
    for (int64_t i = t0; i < n4; i += stride) {
      const f32x4 v = reinterpret_cast<const f32x4*>(p)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        mn = fminf(mn, v[e]);
        mx = fmaxf(mx, v[e]);
        nan |= v[e] != v[e];
      }
    }
    done = n4 * 4;
  }
  for (int64_t i = done + t0; i < n; i += stride) {
    const float v = p[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
    nan |= v != v;
  }
}

__global__ __launch_bounds__(MR_THREADS) void k_range(const float* __restrict__ a, int64_t na, const float* __restrict__ b, int64_t nb,
                                                      unsigned* __restrict__ ws) {
  __shared__ float smn[MR_THREADS / 64], smx[MR_THREADS / 64];
  __shared__ int snan[MR_THREADS / 64];
  float mn = __builtin_inff(), mx = -__builtin_inff();
  bool nan = false;
  if (na > 0) mr_scan(a, na, mn, mx, nan);
  if (nb > 0) mr_scan(b, nb, mn, mx, nan);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  const bool any_nan = __any(nan);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    smn[wave] = mn;
    smx[wave] = mx;
    snan[wave] = any_nan;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int f = 0;
    for (int w = 0; w < MR_THREADS / 64; ++w) {
      mn = fminf(mn, smn[w]);
      mx = fmaxf(mx, smx[w]);
      f |= snan[w];
    }
    atomicMin(ws + 0, mr_enc(mn));
    atomicMax(ws + 1, mr_enc(mx));
    if (f) atomicOr(ws + 2, 1u);
  }
}

__global__ void k_range_final(const unsigned* __restrict__ ws, float* __restrict__ out) {
  const bool nan = ws[2] != 0u;
  out[0] = nan ? __builtin_nanf("") : mr_dec(ws[0]);
  out[1] = nan ? __builtin_nanf("") : mr_dec(ws[1]);
}

extern "C" int64_t mud_value_range_ws_bytes(void) { return 16; }

extern "C" int mud_value_range(const float* a, int64_t na, const float* b, int64_t nb, float* out, void* ws, void* stream) {
  MUD_REQUIRE(na >= 0 && nb >= 0, "mud_value_range: bad sizes");
  MUD_REQUIRE(out && ws && (na == 0 || a) && (nb == 0 || b), "mud_value_range: null pointer");
  MUD_REQUIRE((((uintptr_t)ws) & 3u) == 0 && (((uintptr_t)out) & 3u) == 0, "mud_value_range: ws / out must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int64_t blocks = mud_cdiv(na + nb, (int64_t)MR_THREADS * 16);
  blocks = blocks < 1 ? 1 : (blocks > MR_MAX_BLOCKS ? MR_MAX_BLOCKS : blocks);
  hipLaunchKernelGGL(k_range_init, dim3(1), dim3(1), 0, s, (unsigned*)ws);
  hipLaunchKernelGGL(k_range, dim3((int)blocks), dim3(MR_THREADS), 0, s, a, na, b, nb, (unsigned*)ws);
  hipLaunchKernelGGL(k_range_final, dim3(1), dim3(1), 0, s, (const unsigned*)ws, out);
  MUD_CHECK_LAUNCH("mud_value_range");
  return MUD_OK;
}

// numpy (2.x, fp32 array with weak Python-float scalars): clip((s - lo) / range * 255.0, 0, 255).astype(uint8), every operation
// rounded once in fp32.  The plain operators are IEEE here (HIP's fp32 division is correctly rounded unless -ffast-math or
// -fno-hip-fp32-correctly-rounded-divide-sqrt; neither is used), and contraction is off so the multiply cannot fuse.
__device__ __forceinline__ unsigned char mr_quant(float v, float lo, float range) {
#pragma clang fp contract(off)
  float t = (v - lo) / range * 255.0f;
  t = fminf(fmaxf(t, 0.0f), 255.0f);
  return (unsigned char)(int)t;     // truncation toward zero, like astype(uint8) of a value in [0, 255]
}

__global__ __launch_bounds__(MR_THREADS) void k_quantize_u8(const float* __restrict__ x, int64_t n, float lo, float range,
                                                            unsigned char* __restrict__ out, int vec) {
  const int64_t stride = (int64_t)gridDim.x * MR_THREADS;
  const int64_t t0 = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  int64_t done = 0;
  if (vec) {                        // x 16-byte and out 4-byte aligned: one float4 in, one uchar4 out per lane
    const int64_t n4 = n / 4;
    for (int64_t i = t0; i < n4; i += stride) {
      const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
      uchar4 q;
      q.x = mr_quant(v[0], lo, range);
      q.y = mr_quant(v[1], lo, range);
      q.z = mr_quant(v[2], lo, range);
      q.w = mr_quant(v[3], lo, range);
      reinterpret_cast<uchar4*>(out)[i] = q;
    }
    done = n4 * 4;
  }
  for (int64_t i = done + t0; i < n; i += stride) out[i] = mr_quant(x[i], lo, range);
}

extern "C" int mud_quantize_u8(const float* x, int64_t n, float lo, float range, uint8_t* out, void* stream) {
  MUD_REQUIRE(n >= 0, "mud_quantize_u8: bad size");
  MUD_REQUIRE(range > 0.0f && range <= 3.402823466e38f, "mud_quantize_u8: range must be finite and > 0 (got %g)", (double)range);
  if (n == 0) return MUD_OK;
  MUD_REQUIRE(x && out, "mud_quantize_u8: null pointer");
  const int vec = mud_aligned16(x) && (((uintptr_t)out) & 3u) == 0;
  int64_t blocks = mud_cdiv(n, (int64_t)MR_THREADS * 4);
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(k_quantize_u8, dim3((int)blocks), dim3(MR_THREADS), 0, (hipStream_t)stream, x, n, lo, range, out, vec);
  MUD_CHECK_LAUNCH("mud_quantize_u8");
  return MUD_OK;
}

// ---- per-slice sums: sse = sum (g-p)^2, sae = sum |g-p| (int64), ssim_sum = sum of the per-pixel SSIM over the (H-6)x(W-6) interior
//
// Workgroup (slice, band, column tile).  Lane t reads column tx*SM_OUT_COLS + t of the slice and walks the band's rows keeping the
// 7-row running column sums of q, r, q^2, r^2, q*r in registers; after each row the column sums go to LDS (double-buffered: one
// barrier per row) and lane t < SM_OUT_COLS adds the 7 columns t..t+6 for the output pixel at column tx*SM_OUT_COLS + t + 3.
// Bands split the interior rows [3, H-3) into SM_BAND rows each; tiles split the interior columns into SM_OUT_COLS each.  The sse /
// sae of a pixel is counted by exactly one lane: the band that owns its row (band 0 also owns rows 0-2, the last band rows H-3..H-1)
// and the tile whose first SM_OUT_COLS lanes read its column (the last tile also owns the columns of its 6 halo lanes).
#define SM_BAND 16
#define SM_OUT_COLS (MR_THREADS - 6)

__global__ __launch_bounds__(MR_THREADS) void k_slice_metrics_u8(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ gt,
                                                                 int H, int W, int nb, int ntx, int64_t* __restrict__ part_sse,
                                                                 int64_t* __restrict__ part_sae, double* __restrict__ part_ss) {
  __shared__ int cs[2][5][MR_THREADS];
  __shared__ int red_i[2][MR_THREADS / 64];
  __shared__ double red_d[MR_THREADS / 64];
  const int t = threadIdx.x;
  const int tx = blockIdx.x % ntx;
  const int band = (blockIdx.x / ntx) % nb;
  const int64_t s = (int64_t)blockIdx.x / ((int64_t)ntx * nb);
  const int xs = tx * SM_OUT_COLS + t;
  const bool col_in = xs < W;
  const bool col_err = col_in && (t < SM_OUT_COLS || tx == ntx - 1);
  const bool out_col = t < SM_OUT_COLS && xs < W - 6;               // output pixel x = xs + 3 lies in [3, W-3)
  const int yc0 = 3 + band * SM_BAND, yc1 = min(yc0 + SM_BAND, H - 3);
  const int e_lo = band == 0 ? 0 : yc0, e_hi = band == nb - 1 ? H : yc1;
  const int y0 = yc0 - 3, y1 = yc1 + 3;                              // rows read: [y0, y1), y1 <= H
  const unsigned char* ps = pred + s * H * W + xs;
  const unsigned char* gs = gt + s * H * W + xs;

  int wq[7], wr[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) wq[i] = wr[i] = 0;
  int sq = 0, sr = 0, sqq = 0, srr = 0, sqr = 0, sse = 0, sae = 0;
  double ss = 0.0;
  const double C1 = (0.01 * 0.01) * (12495.0 * 12495.0);             // c1 * (49*255)^2
  const double C2 = (0.03 * 0.03) * (49.0 * 48.0 * 255.0 * 255.0);   // c2 * 49*48*255^2
  int qn = 0, rn = 0;
  if (col_in) {
    qn = ps[(int64_t)y0 * W];
    rn = gs[(int64_t)y0 * W];
  }
  for (int y = y0; y < y1; ++y) {
    const int q = qn, r = rn;
    if (col_in && y + 1 < y1) {                                      // next row's load in flight across this row's barrier
      qn = ps[(int64_t)(y + 1) * W];
      rn = gs[(int64_t)(y + 1) * W];
    }
    if (col_err && y >= e_lo && y < e_hi) {
      const int d = r - q;
      sse += d * d;
      sae += d < 0 ? -d : d;
    }
    const int oq = wq[0], orr = wr[0];                               // row y-7 leaves the window (zero while k < 7)
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      wq[i] = wq[i + 1];
      wr[i] = wr[i + 1];
    }
    wq[6] = q;
    wr[6] = r;
    sq += q - oq;
    sr += r - orr;
    sqq += q * q - oq * oq;
    srr += r * r - orr * orr;
    sqr += q * r - oq * orr;
    if (y - y0 >= 6) {                                               // window rows y-6..y complete: centre row y-3
      int(*c)[MR_THREADS] = cs[(y - y0) & 1];
      c[0][t] = sq;
      c[1][t] = sr;
      c[2][t] = sqq;
      c[3][t] = srr;
      c[4][t] = sqr;
      __syncthreads();
      if (out_col) {
        int Sq = 0, Sr = 0, Sqq = 0, Srr = 0, Sqr = 0;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
          Sq += c[0][t + j];
          Sr += c[1][t + j];
          Sqq += c[2][t + j];
          Srr += c[3][t + j];
          Sqr += c[4][t + j];
        }
        // with mu = S/(49*255), var = 49/48 (S2/(49*255^2) - mu^2): both factors of numerator and denominator scale by
        // (49*255)^2 and 49*48*255^2 respectively, leaving integer terms (all < 2^31) and the two scaled constants
        const int a1 = 2 * Sq * Sr, b1 = Sq * Sq + Sr * Sr;
        const int a2 = 2 * (49 * Sqr - Sq * Sr), b2 = (49 * Sqq - Sq * Sq) + (49 * Srr - Sr * Sr);
        ss += (((double)a1 + C1) * ((double)a2 + C2)) / (((double)b1 + C1) * ((double)b2 + C2));
      }
    }
  }
  // fixed-order workgroup reduction: butterflies per wave, then the waves in index order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sse += __shfl_xor(sse, o, 64);
    sae += __shfl_xor(sae, o, 64);
  }
  ss = mud_wave_sum(ss);
  const int lane = t & 63, wave = t >> 6;
  if (lane == 0) {
    red_i[0][wave] = sse;                                            // <= 64 lanes * 22 rows * 255^2 per wave: fits int32
    red_i[1][wave] = sae;
    red_d[wave] = ss;
  }
  __syncthreads();
  if (t == 0) {
    int64_t e2 = 0, e1 = 0;
    double acc = 0.0;
    for (int w = 0; w < MR_THREADS / 64; ++w) {
      e2 += red_i[0][w];
      e1 += red_i[1][w];
      acc += red_d[w];
    }
    const int64_t slot = s * ((int64_t)nb * ntx) + (int64_t)band * ntx + tx;
    part_sse[slot] = e2;
    part_sae[slot] = e1;
    part_ss[slot] = acc;
  }
}

// one lane per slice: the slice's partials in (band, tile) order
__global__ __launch_bounds__(MR_THREADS) void k_slice_metrics_final(const int64_t* __restrict__ part_sse, const int64_t* __restrict__ part_sae,
                                                                    const double* __restrict__ part_ss, int n, int parts,
                                                                    int64_t* __restrict__ sse, int64_t* __restrict__ sae,
                                                                    double* __restrict__ ssim_sum) {
  const int i = blockIdx.x * MR_THREADS + threadIdx.x;
  if (i >= n) return;
  int64_t e2 = 0, e1 = 0;
  double acc = 0.0;
  for (int k = 0; k < parts; ++k) {
    const int64_t slot = (int64_t)i * parts + k;
    e2 += part_sse[slot];
    e1 += part_sae[slot];
    acc += part_ss[slot];
  }
  sse[i] = e2;
  sae[i] = e1;
  ssim_sum[i] = acc;
}

static int64_t sm_parts(int H, int W) { return mud_cdiv(H - 6, SM_BAND) * mud_cdiv(W - 6, SM_OUT_COLS); }

extern "C" int64_t mud_slice_metrics_ws_bytes(int n, int H, int W) {
  if (n < 0 || H < 7 || W < 7) return -1;
  return (int64_t)n * sm_parts(H, W) * 24;
}

extern "C" int mud_slice_metrics_u8(const uint8_t* pred, const uint8_t* gt, int n, int H, int W, int64_t* sse, int64_t* sae,
                                    double* ssim_sum, void* ws, int64_t ws_bytes, void* stream) {
  MUD_REQUIRE(n >= 0 && H >= 7 && W >= 7, "mud_slice_metrics_u8: need n >= 0 and H, W >= 7 (got n=%d H=%d W=%d)", n, H, W);
  MUD_REQUIRE((int64_t)H * W <= (1ll << 40), "mud_slice_metrics_u8: slice too large (%d x %d)", H, W);
  if (n == 0) return MUD_OK;
  MUD_REQUIRE(pred && gt && sse && sae && ssim_sum && ws, "mud_slice_metrics_u8: null pointer");
  MUD_REQUIRE(ws_bytes >= mud_slice_metrics_ws_bytes(n, H, W), "mud_slice_metrics_u8: ws holds %lld bytes, needs %lld",
              (long long)ws_bytes, (long long)mud_slice_metrics_ws_bytes(n, H, W));
  MUD_REQUIRE((((uintptr_t)ws) & 7u) == 0 && (((uintptr_t)sse) & 7u) == 0 && (((uintptr_t)sae) & 7u) == 0 && (((uintptr_t)ssim_sum) & 7u) == 0,
              "mud_slice_metrics_u8: ws and outputs must be 8-byte aligned");
  const int nb = (int)mud_cdiv(H - 6, SM_BAND), ntx = (int)mud_cdiv(W - 6, SM_OUT_COLS);
  const int64_t parts = (int64_t)nb * ntx, blocks = parts * n;
  MUD_REQUIRE(blocks <= 0x7fffffff, "mud_slice_metrics_u8: too many workgroups (%lld)", (long long)blocks);
  int64_t* p_sse = (int64_t*)ws;
  int64_t* p_sae = p_sse + parts * n;
  double* p_ss = (double*)(p_sae + parts * n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_slice_metrics_u8, dim3((unsigned)blocks), dim3(MR_THREADS), 0, st, pred, gt, H, W, nb, ntx, p_sse, p_sae, p_ss);
  hipLaunchKernelGGL(k_slice_metrics_final, dim3((unsigned)mud_cdiv(n, MR_THREADS)), dim3(MR_THREADS), 0, st, (const int64_t*)p_sse,
                     (const int64_t*)p_sae, (const double*)p_ss, n, (int)parts, sse, sae, ssim_sum);
  MUD_CHECK_LAUNCH("mud_slice_metrics_u8");
  return MUD_OK;
}
