// LPIPS (AlexNet backbone, lpips v0.1, the reference's tools/metric_calc.py:50-51) of uint8 image pairs on the device
// (include/mudiff_hip.h: mud_lpips_packed_bytes, mud_lpips_pack, mud_lpips_ws_bytes, mud_lpips_u8).
//
// Pred and gt images run through the same launches as one batch of 2n images (pred 0..n-1, gt n..2n-1):
//  - conv1..conv5 (torchvision AlexNet features[0:12]) are implicit GEMMs on the fp32-input MFMA v_mfma_f32_32x32x2_f32: every
//    output is a k-ordered fp32 fma chain (exact fp32 arithmetic, no reduced-precision operand), bias and ReLU in the epilogue.
//    conv1 stages straight from the uint8 image through the 768-entry table of the input scaling (ScalingLayer of lpips,
//    built on the host); the others read NHWC fp32 features.  An output pixel's value does not depend on where it lies in a
//    tile or which images share the launch.
//  - 3x3 / stride-2 max pools are their own launches.
//  - the head (per-pixel channel normalisation of both images, squared difference, the lin{l} 1x1 dot product) runs in fp64 on
//    each tap right after its conv, one fp64 partial per (slice, tap, pixel block); a last pass adds each slice's partials in
//    block order and divides by the tap's pixel count.  No float atomics: results are bit-identical run to run and a slice's
//    result does not depend on which other slices share its launch.  Identical images give exactly 0.
#include "mud_common.h"

#define LP_THREADS 256
#define LP_BM 128                 // output pixels per conv workgroup (4 waves x 32)
#define LP_BN 64                  // output channels per conv workgroup (2 MFMA tiles of 32 per wave)
#define LP_BK 32                  // reduction depth of one staged tile
#define LP_SA (LP_BM + 32)        // LDS row strides: the two k rows an MFMA operand read touches land 32 banks apart
#define LP_SB (LP_BN + 32)
#define LP_HEAD_PIX 64            // pixels per head workgroup (16 per wave)
#define LP_TAB 768                // input table: 3 channels x 256 levels

// ---- network geometry: conv l has Cin -> Cout, ks x ks, stride, pad; Kpad = ks*ks*Cin rounded up to LP_BK
static const int LP_CIN[5] = {3, 64, 192, 384, 256};
static const int LP_COUT[5] = {64, 192, 384, 256, 256};
static const int LP_KS[5] = {11, 5, 3, 3, 3};
static const int LP_STRIDE[5] = {4, 1, 1, 1, 1};
static const int LP_PAD[5] = {2, 2, 1, 1, 1};

static int64_t lp_align64(int64_t f) { return (f + 63) / 64 * 64; }     // segments start on 256-byte boundaries
static int lp_kpad(int l) { return (int)mud_cdiv((int64_t)LP_KS[l] * LP_KS[l] * LP_CIN[l], LP_BK) * LP_BK; }

// packed layout (floats): table[768] | per conv: w[Kpad][Cout], b[Cout] | per tap: lin[C]
struct lp_layout {
  int64_t tab, w[5], b[5], lin[5], total;
};
static lp_layout lp_offsets() {
  lp_layout L;
  int64_t o = 0;
  L.tab = o;
  o += lp_align64(LP_TAB);
  for (int l = 0; l < 5; ++l) {
    L.w[l] = o;
    o += lp_align64((int64_t)lp_kpad(l) * LP_COUT[l]);
    L.b[l] = o;
    o += lp_align64(LP_COUT[l]);
  }
  for (int l = 0; l < 5; ++l) {
    L.lin[l] = o;
    o += lp_align64(LP_COUT[l]);
  }
  L.total = o;
  return L;
}

// spatial sizes: conv l's input (hi, wi) and output (ho, wo); tap l = conv l's output
struct lp_geom {
  int hi[5], wi[5], ho[5], wo[5];
  int64_t x_floats, y_floats;     // per image: the largest map each of the two ping-pong buffers holds
  int64_t parts[5], part_off[5], parts_total;
};
static int lp_pool(int v) { return (v - 3) / 2 + 1; }
static lp_geom lp_geometry(int H, int W) {
  lp_geom g;
  int h = H, w = W;
  for (int l = 0; l < 5; ++l) {
    g.hi[l] = h;
    g.wi[l] = w;
    g.ho[l] = (h + 2 * LP_PAD[l] - LP_KS[l]) / LP_STRIDE[l] + 1;
    g.wo[l] = (w + 2 * LP_PAD[l] - LP_KS[l]) / LP_STRIDE[l] + 1;
    h = g.ho[l];
    w = g.wo[l];
    if (l < 2) {
      h = lp_pool(h);
      w = lp_pool(w);
    }
  }
  // X: relu1, relu2, relu3, relu5; Y: pool1, pool2, relu4
  auto px = [&](int l) { return (int64_t)g.ho[l] * g.wo[l] * LP_COUT[l]; };
  g.x_floats = px(0);
  if (px(1) > g.x_floats) g.x_floats = px(1);
  if (px(2) > g.x_floats) g.x_floats = px(2);
  if (px(4) > g.x_floats) g.x_floats = px(4);
  g.y_floats = (int64_t)g.hi[1] * g.wi[1] * LP_CIN[1];
  if ((int64_t)g.hi[2] * g.wi[2] * LP_CIN[2] > g.y_floats) g.y_floats = (int64_t)g.hi[2] * g.wi[2] * LP_CIN[2];
  if (px(3) > g.y_floats) g.y_floats = px(3);
  g.parts_total = 0;
  for (int l = 0; l < 5; ++l) {
    g.parts[l] = mud_cdiv((int64_t)g.ho[l] * g.wo[l], LP_HEAD_PIX);
    g.part_off[l] = g.parts_total;
    g.parts_total += g.parts[l];
  }
  return g;
}

// ---- weight packing: [Cout][Cin][ks][ks] (torch) -> [Kpad][Cout] with k = (kh*ks + kw)*Cin + ci, zero rows k >= ks*ks*Cin
__global__ __launch_bounds__(LP_THREADS) void k_lp_pack_conv(const float* __restrict__ w, int Cout, int Cin, int ks, int Kpad,
                                                             float* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
  if (i >= (int64_t)Kpad * Cout) return;
  const int co = (int)(i % Cout), k = (int)(i / Cout);
  float v = 0.0f;
  if (k < ks * ks * Cin) {
    const int ci = k % Cin, khw = k / Cin, kh = khw / ks, kw = khw % ks;
    v = w[(((int64_t)co * Cin + ci) * ks + kh) * ks + kw];
  }
  dst[i] = v;
}

__global__ __launch_bounds__(LP_THREADS) void k_lp_copy(const float* __restrict__ src, int n, float* __restrict__ dst) {
  const int i = blockIdx.x * LP_THREADS + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

extern "C" int64_t mud_lpips_packed_bytes(void) { return lp_offsets().total * 4; }

extern "C" int mud_lpips_pack(const float* table, void* const* conv_w, void* const* conv_b, void* const* lin_w, void* packed, void* stream) {
  MUD_REQUIRE(table && conv_w && conv_b && lin_w && packed, "mud_lpips_pack: null pointer");
  for (int l = 0; l < 5; ++l) MUD_REQUIRE(conv_w[l] && conv_b[l] && lin_w[l], "mud_lpips_pack: null weight pointer for layer %d", l + 1);
  MUD_REQUIRE(mud_aligned16(packed), "mud_lpips_pack: packed must be 16-byte aligned");
  const lp_layout L = lp_offsets();
  float* p = (float*)packed;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_lp_copy, dim3((unsigned)mud_cdiv(LP_TAB, LP_THREADS)), dim3(LP_THREADS), 0, s, table, LP_TAB, p + L.tab);
  for (int l = 0; l < 5; ++l) {
    const int64_t nw = (int64_t)lp_kpad(l) * LP_COUT[l];
    hipLaunchKernelGGL(k_lp_pack_conv, dim3((unsigned)mud_cdiv(nw, LP_THREADS)), dim3(LP_THREADS), 0, s, (const float*)conv_w[l], LP_COUT[l],
                       LP_CIN[l], LP_KS[l], lp_kpad(l), p + L.w[l]);
    hipLaunchKernelGGL(k_lp_copy, dim3((unsigned)mud_cdiv(LP_COUT[l], LP_THREADS)), dim3(LP_THREADS), 0, s, (const float*)conv_b[l], LP_COUT[l],
                       p + L.b[l]);
    hipLaunchKernelGGL(k_lp_copy, dim3((unsigned)mud_cdiv(LP_COUT[l], LP_THREADS)), dim3(LP_THREADS), 0, s, (const float*)lin_w[l], LP_COUT[l],
                       p + L.lin[l]);
  }
  MUD_CHECK_LAUNCH("mud_lpips_pack");
  return MUD_OK;
}

// ---- implicit-GEMM convolution, D[m][co] = relu(bias[co] + sum_k A[m][k] W[k][co]), m = (image, oh, ow), NHWC out [M][Cout].
// Workgroup tile LP_BM x LP_BN, wave w owns rows 32w..32w+31 and both 32-column halves.  Tiles of LP_BK reduction rows are
// staged global -> registers (one tile ahead) -> LDS as As[k][m], Bs[k][co].
// FIRST: the input is the uint8 image [B][H][W], A[m][k] = tab[c*256 + img[ih][iw]] with k = (kh*11 + kw)*3 + c (zero padding
// and zero rows k >= 363); otherwise NHWC fp32 [B][H][W][Cin] with Cin % LP_BK == 0, so a tile is one (kh, kw) and LP_BK channels.
struct lp_conv_args {
  const void* x;
  int H, W, Cin, Ho, Wo, ks, stride, pad, Kpad, Cout, M;
  const float* wt;
  const float* bias;
  const float* tab;
  float* out;
};

template <bool FIRST>
__global__ __launch_bounds__(LP_THREADS) void k_lp_conv(lp_conv_args a) {
  __shared__ float As[LP_BK * LP_SA];
  __shared__ float Bs[LP_BK * LP_SB];
  __shared__ int s_off[LP_BM], s_ih[LP_BM], s_iw[LP_BM];
  __shared__ float s_tab[FIRST ? LP_TAB : 1];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.x * LP_BM, n0 = blockIdx.y * LP_BN;
  const int HoWo = a.Ho * a.Wo;
  if (t < LP_BM) {
    const int m = m0 + t;
    if (m < a.M) {
      const int img = m / HoWo, r = m - img * HoWo, oh = r / a.Wo, ow = r - oh * a.Wo;
      s_off[t] = img * a.H * a.W;
      s_ih[t] = oh * a.stride - a.pad;
      s_iw[t] = ow * a.stride - a.pad;
    } else {
      s_off[t] = 0;
      s_ih[t] = -(1 << 28);                  // never in bounds: the row stages zeros
      s_iw[t] = 0;
    }
  }
  if (FIRST)
    for (int i = t; i < LP_TAB; i += LP_THREADS) s_tab[i] = a.tab[i];
  __syncthreads();

  float ra[16];                              // staged A: FIRST 16 scalars, else 4 float4
  f32x4 rb[2];
  const int ntiles = a.Kpad / LP_BK;

  auto load = [&](int tile) {
    const int k0 = tile * LP_BK;
    if (FIRST) {
      const unsigned char* img = (const unsigned char*)a.x;
      const int kl = t >> 3, k = k0 + kl;
      const bool kin = k < a.ks * a.ks * 3;
      const int c = k % 3, khw = k / 3, kh = khw / a.ks, kw = khw % a.ks;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int p = (t & 7) + 8 * j;
        const int ih = s_ih[p] + kh, iw = s_iw[p] + kw;
        float v = 0.0f;
        if (kin && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) v = s_tab[c * 256 + img[(int64_t)s_off[p] + ih * a.W + iw]];
        ra[j] = v;
      }
    } else {
      const float* x = (const float*)a.x;
      const int khw = k0 / a.Cin, c0 = k0 - khw * a.Cin, kh = khw / a.ks, kw = khw - kh * a.ks;
      const int q = t & 7;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int p = (t >> 3) + 32 * j;
        const int ih = s_ih[p] + kh, iw = s_iw[p] + kw;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W)
          v = *reinterpret_cast<const f32x4*>(x + ((int64_t)s_off[p] + ih * a.W + iw) * a.Cin + c0 + 4 * q);
        ra[4 * j + 0] = v[0];
        ra[4 * j + 1] = v[1];
        ra[4 * j + 2] = v[2];
        ra[4 * j + 3] = v[3];
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = t + LP_THREADS * j, k = idx >> 4, n4 = idx & 15;
      rb[j] = *reinterpret_cast<const f32x4*>(a.wt + (int64_t)(k0 + k) * a.Cout + n0 + 4 * n4);
    }
  };
  auto store = [&]() {
    if (FIRST) {
      const int kl = t >> 3;
#pragma unroll
      for (int j = 0; j < 16; ++j) As[kl * LP_SA + (t & 7) + 8 * j] = ra[j];
    } else {
      const int q = t & 7;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int p = (t >> 3) + 32 * j;
#pragma unroll
        for (int e = 0; e < 4; ++e) As[(4 * q + e) * LP_SA + p] = ra[4 * j + e];
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = t + LP_THREADS * j, k = idx >> 4, n4 = idx & 15;
      *reinterpret_cast<f32x4*>(Bs + k * LP_SB + 4 * n4) = rb[j];
    }
  };

  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
  load(0);
  const int kr = lane >> 5, col = lane & 31;
  for (int tile = 0; tile < ntiles; ++tile) {
    store();
    __syncthreads();
    if (tile + 1 < ntiles) load(tile + 1);   // next tile's global loads in flight during this tile's MFMAs
#pragma unroll
    for (int kk = 0; kk < LP_BK / 2; ++kk) {
      const int k = 2 * kk + kr;
      const float av = As[k * LP_SA + 32 * wave + col];
      const float b0 = Bs[k * LP_SB + col], b1 = Bs[k * LP_SB + 32 + col];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc1, 0, 0, 0);
    }
    __syncthreads();
  }
  // epilogue: C/D map row = (r&3) + 8(r>>2) + 4(lane>>5) (pixel), col = lane&31 (channel)
  const float bias0 = a.bias[n0 + col], bias1 = a.bias[n0 + 32 + col];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * kr;
    if (m < a.M) {
      float* o = a.out + (int64_t)m * a.Cout + n0 + col;
      o[0] = fmaxf(acc0[r] + bias0, 0.0f);
      o[32] = fmaxf(acc1[r] + bias1, 0.0f);
    }
  }
}

// ---- 3x3 / stride-2 max pool, no padding, NHWC: one float4 of channels per lane
__global__ __launch_bounds__(LP_THREADS) void k_lp_maxpool(const float* __restrict__ x, int B, int H, int W, int C, int Ho, int Wo,
                                                           float* __restrict__ out) {
  const int C4 = C / 4;
  const int64_t i = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
  if (i >= (int64_t)B * Ho * Wo * C4) return;
  const int c4 = (int)(i % C4);
  const int64_t pix = i / C4;
  const int ow = (int)(pix % Wo), oh = (int)((pix / Wo) % Ho);
  const int64_t img = pix / ((int64_t)Wo * Ho);
  const float* base = x + ((img * H + 2 * oh) * W + 2 * ow) * C + 4 * c4;
  f32x4 m = *reinterpret_cast<const f32x4*>(base);
#pragma unroll
  for (int dh = 0; dh < 3; ++dh)
#pragma unroll
    for (int dw = 0; dw < 3; ++dw) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(base + ((int64_t)dh * W + dw) * C);
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[e]);
    }
  *reinterpret_cast<f32x4*>(out + pix * C + 4 * c4) = m;
}

// ---- head of one tap: f [2n][P][C] (pred images first); partial[i][part_off + blk] = sum over the block's pixels p of
// sum_c w[c] (f0[c]/(|f0| + 1e-10) - f1[c]/(|f1| + 1e-10))^2, in fp64.  One wave per pixel (lanes over channels, C % 64 == 0),
// each wave's pixels in order, then the waves in index order.
__global__ __launch_bounds__(LP_THREADS) void k_lp_head(const float* __restrict__ f, int n, int P, int C, int nblk, const float* __restrict__ lin,
                                                        double* __restrict__ part, int64_t part_ld, int64_t part_off) {
  __shared__ double red[LP_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = blockIdx.x / nblk;
  const int blk = blockIdx.x % nblk;
  const int p1 = min(P, (blk + 1) * LP_HEAD_PIX);
  double acc = 0.0;
  for (int p = blk * LP_HEAD_PIX + wave; p < p1; p += LP_THREADS / 64) {
    const float* f0 = f + (i * P + p) * C;
    const float* f1 = f + ((i + n) * P + p) * C;
    double s0 = 0.0, s1 = 0.0;
    for (int c = lane; c < C; c += 64) {
      const double u = f0[c], v = f1[c];
      s0 += u * u;
      s1 += v * v;
    }
    s0 = mud_wave_sum(s0);
    s1 = mud_wave_sum(s1);
    const double r0 = 1.0 / (sqrt(s0) + 1e-10), r1 = 1.0 / (sqrt(s1) + 1e-10);
    double d = 0.0;
    for (int c = lane; c < C; c += 64) {
#pragma clang fp contract(off)      // no fma here: with identical images both products round alike and e is exactly 0
      const double e = (double)f0[c] * r0 - (double)f1[c] * r1;
      d += (double)lin[c] * e * e;
    }
    acc += mud_wave_sum(d);
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < LP_THREADS / 64; ++w) s += red[w];
    part[i * part_ld + part_off + blk] = s;
  }
}

// one lane per (slice, tap): the partials in block order, then the spatial mean
struct lp_final_args {
  int64_t parts[5], part_off[5];
  double npix[5];
};
__global__ __launch_bounds__(LP_THREADS) void k_lp_final(const double* __restrict__ part, int n, int64_t part_ld, lp_final_args g,
                                                         double* __restrict__ out) {
  const int idx = blockIdx.x * LP_THREADS + threadIdx.x;
  if (idx >= n * 5) return;
  const int i = idx / 5, l = idx % 5;
  int64_t off = 0, cnt = 0;
  double np = 1.0;
#pragma unroll
  for (int k = 0; k < 5; ++k)
    if (k == l) {
      off = g.part_off[k];
      cnt = g.parts[k];
      np = g.npix[k];
    }
  const double* p = part + (int64_t)i * part_ld + off;
  double s = 0.0;
  for (int64_t b = 0; b < cnt; ++b) s += p[b];
  out[idx] = s / np;
}

// workspace: X [2n][x_floats] | Y [2n][y_floats] | partials [n][parts_total] (fp64), each 256-byte aligned
struct lp_ws {
  int64_t x, y, part, total;
};
static lp_ws lp_ws_layout(int n, const lp_geom& g) {
  lp_ws w;
  w.x = 0;
  w.y = w.x + lp_align64(2 * (int64_t)n * g.x_floats) * 4;
  w.part = w.y + lp_align64(2 * (int64_t)n * g.y_floats) * 4;
  w.total = w.part + lp_align64((int64_t)n * g.parts_total * 2) * 4;
  return w;
}

extern "C" int64_t mud_lpips_ws_bytes(int n, int H, int W) {
  if (n < 0 || H < 31 || W < 31) return -1;
  return lp_ws_layout(n, lp_geometry(H, W)).total;
}

extern "C" int mud_lpips_u8(const uint8_t* pred, const uint8_t* gt, int n, int H, int W, const void* packed, double* out, void* ws,
                            int64_t ws_bytes, void* stream) {
  MUD_REQUIRE(n >= 0 && H >= 31 && W >= 31, "mud_lpips_u8: need n >= 0 and H, W >= 31 (got n=%d H=%d W=%d)", n, H, W);
  MUD_REQUIRE(pred && gt && packed && out && ws, "mud_lpips_u8: null pointer");
  const lp_geom g = lp_geometry(H, W);
  const lp_ws L = lp_ws_layout(n, g);
  MUD_REQUIRE(ws_bytes >= L.total, "mud_lpips_u8: ws holds %lld bytes, needs %lld", (long long)ws_bytes, (long long)L.total);
  MUD_REQUIRE(mud_aligned16(packed) && mud_aligned16(ws) && (((uintptr_t)out) & 7u) == 0,
              "mud_lpips_u8: packed and ws must be 16-byte aligned, out 8-byte aligned");
  // every index inside a launch is 32-bit: the largest map of the batch and the staged uint8 input must stay below 2^31 elements
  MUD_REQUIRE(2 * (int64_t)n * g.x_floats < (1ll << 31) && 2 * (int64_t)n * g.y_floats < (1ll << 31) && 2 * (int64_t)n * H * W < (1ll << 31),
              "mud_lpips_u8: batch too large (n=%d at %dx%d): split it", n, H, W);
  if (n == 0) return MUD_OK;
  hipStream_t s = (hipStream_t)stream;
  const lp_layout P = lp_offsets();
  const float* pk = (const float*)packed;
  float* X = (float*)((char*)ws + L.x);
  float* Y = (float*)((char*)ws + L.y);
  double* part = (double*)((char*)ws + L.part);
  const int B = 2 * n;

  // pred and gt side by side in one uint8 batch: the first B*H*W bytes of Y are free until pool1 writes there
  uint8_t* img = (uint8_t*)Y;
  MUD_REQUIRE(g.y_floats * 4 >= (int64_t)H * W, "mud_lpips_u8: internal: staging buffer too small");
  if (hipMemcpyAsync(img, pred, (size_t)n * H * W, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemcpyAsync(img + (size_t)n * H * W, gt, (size_t)n * H * W, hipMemcpyDeviceToDevice, s) != hipSuccess) {
    mud_set_error("mud_lpips_u8: staging copy failed: %s", hipGetErrorString(hipGetLastError()));
    return MUD_ERR_LAUNCH;
  }

  auto conv = [&](int l, const void* x, float* o) {
    lp_conv_args a;
    a.x = x;
    a.H = g.hi[l];
    a.W = g.wi[l];
    a.Cin = LP_CIN[l];
    a.Ho = g.ho[l];
    a.Wo = g.wo[l];
    a.ks = LP_KS[l];
    a.stride = LP_STRIDE[l];
    a.pad = LP_PAD[l];
    a.Kpad = lp_kpad(l);
    a.Cout = LP_COUT[l];
    a.M = B * g.ho[l] * g.wo[l];
    a.wt = pk + P.w[l];
    a.bias = pk + P.b[l];
    a.tab = pk + P.tab;
    a.out = o;
    const dim3 grid((unsigned)mud_cdiv(a.M, LP_BM), (unsigned)(a.Cout / LP_BN));
    if (l == 0)
      hipLaunchKernelGGL(k_lp_conv<true>, grid, dim3(LP_THREADS), 0, s, a);
    else
      hipLaunchKernelGGL(k_lp_conv<false>, grid, dim3(LP_THREADS), 0, s, a);
  };
  auto pool = [&](int l, const float* x, float* o) {     // conv l's output -> conv l+1's input
    const int64_t work = (int64_t)B * g.hi[l + 1] * g.wi[l + 1] * (LP_COUT[l] / 4);
    hipLaunchKernelGGL(k_lp_maxpool, dim3((unsigned)mud_cdiv(work, LP_THREADS)), dim3(LP_THREADS), 0, s, x, B, g.ho[l], g.wo[l], LP_COUT[l],
                       g.hi[l + 1], g.wi[l + 1], o);
  };
  auto head = [&](int l, const float* f) {
    const int P_l = g.ho[l] * g.wo[l];
    hipLaunchKernelGGL(k_lp_head, dim3((unsigned)(n * g.parts[l])), dim3(LP_THREADS), 0, s, f, n, P_l, LP_COUT[l], (int)g.parts[l],
                       pk + P.lin[l], part, g.parts_total, g.part_off[l]);
  };
  MUD_REQUIRE((int64_t)n * g.parts[0] <= 0x7fffffff, "mud_lpips_u8: too many workgroups");
  conv(0, img, X);
  head(0, X);
  pool(0, X, Y);
  conv(1, Y, X);
  head(1, X);
  pool(1, X, Y);
  conv(2, Y, X);
  head(2, X);
  conv(3, X, Y);
  head(3, Y);
  conv(4, Y, X);
  head(4, X);
  lp_final_args fa;
  for (int l = 0; l < 5; ++l) {
    fa.parts[l] = g.parts[l];
    fa.part_off[l] = g.part_off[l];
    fa.npix[l] = (double)g.ho[l] * g.wo[l];
  }
  hipLaunchKernelGGL(k_lp_final, dim3((unsigned)mud_cdiv((int64_t)n * 5, LP_THREADS)), dim3(LP_THREADS), 0, s, (const double*)part, n,
                     g.parts_total, fa, out);
  MUD_CHECK_LAUNCH("mud_lpips_u8");
  return MUD_OK;
}
