// Non-local-means denoising of the volume pipeline's inputs (--denoise; include/mudiff_hip.h: mud_volume_denoise_*;
// mudiff_hip.volume_denoise).
//
// Three kernels.  The noise level: the pseudo-residual of every voxel against its six face neighbours as the uint32 bits of |eps| (1),
// then the exact lower median of those keys by four passes of a 256-bin radix histogram, the host picking the bin after each (2).  The
// estimate itself (3): one workgroup owns a 32 x 8 x 4 tile of output voxels and stages the tile with a halo of search + patch voxels
// per side in LDS once, as the fp32 values (NaN outside the volume: a voxel is valid iff its value is finite).  Per search offset t the
// workgroup writes D_t = (v(x) - v(x + t))^2 over the tile grown by the patch radius into LDS once (-1 where x or x + t is not valid),
// and every thread box-sums the (2 r + 1)^3 entries around each of its four voxels, z outermost and x fastest: d2 is the sum in the
// order of tests/volume_denoise_ref.py, with half the LDS reads of a per-patch subtraction and no subtract / multiply per patch voxel.
// Two D planes alternate, so one barrier per offset.  Every fp32 / fp64 expression is evaluated uncontracted in the restatement's order;
// only expf is the math library's.  The estimation's sums are integer counts: two runs give the same bits.
#include "volume_common.h"

#define VD_VX 4                                // a thread owns VD_VX consecutive voxels of a row of the VI_TX x VI_TY x VI_TZ tile
#define VD_MAX_SEARCH 5
#define VD_MAX_PATCH 2
#define VD_MAX_LDS (160 * 1024)
#define VD_SKIP 0xFFFFFFFFu                    // the key of a voxel outside the estimation set

static_assert(VI_TX / VD_VX * VI_TY * VI_TZ == VI_THREADS, "one thread per VD_VX voxels of the tile");

// ---- 1: keys[i] = bits of |eps|, eps = sqrtf(6/7) * (v - (sum of the six face neighbours) / 6), over the voxels that are > 0 with six
// neighbours inside the volume, valid and > 0; VD_SKIP elsewhere
template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_vd_residual(vi_source src, int X, int Y, int Z, int64_t n, uint32_t* __restrict__ keys) {
#pragma clang fp contract(off)
  const float K = 0.9258200997725514f;         // float32(sqrt(6 / 7))
  VI_GRID_STRIDE(i, n) {
    int x, y, z;
    vi_xyz(i, X, Y, x, y, z);
    uint32_t key = VD_SKIP;
    if (x > 0 && x < X - 1 && y > 0 && y < Y - 1 && z > 0 && z < Z - 1) {
      const int64_t sy = X, sz = (int64_t)X * Y;
      const float v = vi_at<T>(src, i);
      const float a = vi_at<T>(src, i - 1), b = vi_at<T>(src, i + 1), c = vi_at<T>(src, i - sy), d = vi_at<T>(src, i + sy);
      const float e = vi_at<T>(src, i - sz), f = vi_at<T>(src, i + sz);
      const bool ok = vc_finite(v) && v > 0.0f && vc_finite(a) && a > 0.0f && vc_finite(b) && b > 0.0f && vc_finite(c) && c > 0.0f &&
                      vc_finite(d) && d > 0.0f && vc_finite(e) && e > 0.0f && vc_finite(f) && f > 0.0f;
      if (ok) {
        float s = a + b;
        s = s + c;
        s = s + d;
        s = s + e;
        s = s + f;
        const float mean = s / 6.0f;
        const float eps = K * (v - mean);
        key = __float_as_uint(eps) & 0x7FFFFFFFu;
      }
    }
    keys[i] = key;
  }
}

// ---- 2: one pass of the radix select: the counts of byte 3 - pass of the keys whose higher bytes equal `prefix`
__global__ __launch_bounds__(VI_THREADS) void k_vd_select_hist(const uint32_t* __restrict__ keys, int64_t n, uint32_t prefix, int pass,
                                                               uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  // 256 bins, VI_THREADS threads: the shared loops run once per thread.  Chosen over h[threadIdx.x] = 0 written out here: the same 9
  // VGPRs and the same loop over the keys, six scalar / compare instructions more per workgroup outside that loop, one definition fewer
  vc_hist_clear(h, 256);
  const int shift = 24 - 8 * pass;
  VI_GRID_STRIDE(i, n) {
    const uint32_t k = keys[i];
    if (k == VD_SKIP) continue;
    if (pass == 0 || ((k >> shift) >> 8) == prefix) atomicAdd(&h[(k >> shift) & 255u], 1u);
  }
  vc_hist_merge(h, 256, hist);
}

// ---- 3: the estimate
extern __shared__ __attribute__((aligned(16))) float vd_lds[];

template <int R>
struct vd_plane {                              // D_t over the tile grown by R per side; rows padded to a multiple of 4 floats
  static constexpr int DX = VI_TX + 2 * R, DY = VI_TY + 2 * R, DZ = VI_TZ + 2 * R;
  static constexpr int DXP = (DX + 3) / 4 * 4;
  static constexpr int COUNT = DX * DY * DZ, FLOATS = DXP * DY * DZ;
  static constexpr int PER_THREAD = (COUNT + VI_THREADS - 1) / VI_THREADS;
};

static inline int vd_staged_floats(int s, int r) {
  const int H = s + r;
  return ((VI_TX + 2 * H) * (VI_TY + 2 * H) * (VI_TZ + 2 * H) + 3) / 4 * 4;
}

template <typename T, int R>
__global__ __launch_bounds__(VI_THREADS) void k_vd_nlm(vi_source vol, int X, int Y, int Z, int s, int staged, float h, double bias, int rician,
                                                       float* __restrict__ out, uint32_t* __restrict__ zeroed) {
#pragma clang fp contract(off)
  typedef vd_plane<R> P;
  constexpr int W = 2 * R + 1, ROW = VD_VX + 2 * R;
  __shared__ uint32_t nzeroed;                 // the workgroup's count: a histogram of one bin
  const int H = s + R;
  const int SX = VI_TX + 2 * H, SY = VI_TY + 2 * H, SZ = VI_TZ + 2 * H;
  float* S = vd_lds;
  float* D = vd_lds + staged;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * VI_TX, y0 = blockIdx.y * VI_TY, z0 = blockIdx.z * VI_TZ;
  const float nan = __uint_as_float(0x7fc00000u);
  for (int i = tid; i < SX * SY * SZ; i += VI_THREADS) {
    const int row = i / SX, ix = i - row * SX, iz = row / SY, iy = row - iz * SY;
    const int gx = x0 - H + ix, gy = y0 - H + iy, gz = z0 - H + iz;
    float v = nan;
    if (gx >= 0 && gx < X && gy >= 0 && gy < Y && gz >= 0 && gz < Z) v = vi_at<T>(vol, ((int64_t)gz * Y + gy) * X + gx);
    S[i] = v;
  }
  // this thread's entries of a D plane: where they sit in the plane and in the staged tile (the same for every offset)
  int d_at[P::PER_THREAD], s_at[P::PER_THREAD];
#pragma unroll
  for (int k = 0; k < P::PER_THREAD; ++k) {
    const int i = tid + k * VI_THREADS;
    const int row = i / P::DX, dx = i - row * P::DX, dz = row / P::DY, dy = row - dz * P::DY;
    d_at[k] = i < P::COUNT ? (dz * P::DY + dy) * P::DXP + dx : -1;
    s_at[k] = i < P::COUNT ? ((dz + s) * SY + (dy + s)) * SX + (dx + s) : 0;
  }
  const int tx = tid & (VI_TX / VD_VX - 1), ty = (tid / (VI_TX / VD_VX)) & (VI_TY - 1), tz = tid / (VI_TX / VD_VX * VI_TY);
  const int mine = (tz * P::DY + ty) * P::DXP + tx * VD_VX;             // the corner of this thread's first patch in a D plane
  double sw[VD_VX], sa[VD_VX];
  float wmax[VD_VX];
#pragma unroll
  for (int j = 0; j < VD_VX; ++j) sw[j] = 0.0, sa[j] = 0.0, wmax[j] = 0.0f;
  vc_hist_clear(&nzeroed, 1);                  // (its barrier also ends the staging)
  int turn = 0;
  for (int oz = -s; oz <= s; ++oz)
    for (int oy = -s; oy <= s; ++oy)
      for (int ox = -s; ox <= s; ++ox) {
        if (ox == 0 && oy == 0 && oz == 0) continue;
        float* Dp = D + turn * P::FLOATS;
        turn ^= 1;
        const int shift = (oz * SY + oy) * SX + ox;
#pragma unroll
        for (int k = 0; k < P::PER_THREAD; ++k) {
          if (d_at[k] < 0) continue;
          const float a = S[s_at[k]], b = S[s_at[k] + shift];
          const float d = a - b;
          Dp[d_at[k]] = (vc_finite(a) && vc_finite(b)) ? d * d : -1.0f;
        }
        __syncthreads();
        float sum[VD_VX], centre[VD_VX];
        int cnt[VD_VX];
#pragma unroll
        for (int j = 0; j < VD_VX; ++j) sum[j] = 0.0f, cnt[j] = 0, centre[j] = -1.0f;
#pragma unroll
        for (int pz = 0; pz < W; ++pz)
#pragma unroll
          for (int py = 0; py < W; ++py) {
            const float* src = Dp + mine + (pz * P::DY + py) * P::DXP;
            float row[ROW];
            const f32x4 lo = *(const f32x4*)src;
            row[0] = lo[0], row[1] = lo[1], row[2] = lo[2], row[3] = lo[3];
#pragma unroll
            for (int e = 4; e < ROW; ++e) row[e] = src[e];
#pragma unroll
            for (int j = 0; j < VD_VX; ++j)
#pragma unroll
              for (int px = 0; px < W; ++px) {
                const float v = row[j + px];
                if (v >= 0.0f) {
                  sum[j] = sum[j] + v;
                  cnt[j] += 1;
                }
                if (pz == R && py == R && px == R) centre[j] = v;
              }
          }
        const int q = (((tz + H + oz) * SY) + (ty + H + oy)) * SX + tx * VD_VX + H + ox;
#pragma unroll
        for (int j = 0; j < VD_VX; ++j) {
          if (!(centre[j] >= 0.0f)) continue;                           // p or q is not valid, or q is outside the volume
          const float d2 = sum[j] / (float)cnt[j];
          const float w = expf(-(d2 / h));
          double a = (double)S[q + j];
          if (rician) a = a * a;
          const double term = (double)w * a;
          sw[j] = sw[j] + (double)w;
          sa[j] = sa[j] + term;
          wmax[j] = w > wmax[j] ? w : wmax[j];
        }
      }
  uint32_t nz = 0;
  const int gy = y0 + ty, gz = z0 + tz;
#pragma unroll
  for (int j = 0; j < VD_VX; ++j) {
    const int gx = x0 + tx * VD_VX + j;
    if (gx >= X || gy >= Y || gz >= Z) continue;
    const float v = S[((tz + H) * SY + (ty + H)) * SX + tx * VD_VX + j + H];
    float res = v;
    if (vc_finite(v) && v != 0.0f) {
      double a = (double)v;
      if (rician) a = a * a;
      const double wc = wmax[j] > 0.0f ? (double)wmax[j] : 1.0;         // no candidate, or every weight underflowed: the voxel itself
      const double num = sa[j] + wc * a;
      const double den = sw[j] + wc;
      double m = num / den;
      if (rician) {
        m = m - bias;
        m = m > 0.0 ? m : 0.0;
        m = sqrt(m);
      }
      res = (float)m;
      if (res == 0.0f) nz += 1;
    }
    out[((int64_t)gz * Y + gy) * X + gx] = res;
  }
  if (nz) atomicAdd(&nzeroed, nz);
  vc_hist_merge(&nzeroed, 1, zeroed);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------
extern "C" int mud_volume_denoise_residual(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, uint32_t* keys,
                                           void* stream) {
  if (int e = vi_check_volume("mud_volume_denoise_residual", vol, datatype, X, Y, Z)) return e;
  MUD_REQUIRE(keys != nullptr && vi_aligned(keys, 4), "mud_volume_denoise_residual: keys must be a 4-byte aligned pointer");
  const int64_t n = (int64_t)X * Y * Z;
  VI_DISPATCH(datatype, hipLaunchKernelGGL(k_vd_residual<T>, dim3(vi_blocks(n)), dim3(VI_THREADS), 0, (hipStream_t)stream,
                                           vi_source_of(vol, datatype, slope, inter), X, Y, Z, n, keys));
  MUD_CHECK_LAUNCH("mud_volume_denoise_residual");
  return MUD_OK;
}

extern "C" int mud_volume_denoise_select_hist(const uint32_t* keys, int64_t n, uint32_t prefix, int pass, uint32_t* hist, void* stream) {
  MUD_REQUIRE(keys != nullptr && hist != nullptr, "mud_volume_denoise_select_hist: null pointer");
  MUD_REQUIRE(vi_aligned(keys, 4) && vi_aligned(hist, 4), "mud_volume_denoise_select_hist: keys and hist must be 4-byte aligned");
  MUD_REQUIRE(n > 0 && n < ((int64_t)1 << 31), "mud_volume_denoise_select_hist: bad key count %lld", (long long)n);
  MUD_REQUIRE(pass >= 0 && pass <= 3, "mud_volume_denoise_select_hist: pass %d is not in [0, 3]", pass);
  MUD_REQUIRE(pass == 0 ? prefix == 0 : (prefix >> (8 * pass)) == 0, "mud_volume_denoise_select_hist: prefix 0x%x has more than %d bytes", prefix,
              pass);
  hipStream_t s = (hipStream_t)stream;
  if (int e = vi_clear("mud_volume_denoise_select_hist", hist, sizeof(uint32_t) * 256, s)) return e;
  hipLaunchKernelGGL(k_vd_select_hist, dim3(vi_blocks(n)), dim3(VI_THREADS), 0, s, keys, n, prefix, pass, hist);
  MUD_CHECK_LAUNCH("mud_volume_denoise_select_hist");
  return MUD_OK;
}

template <typename T, int R>
static int vd_launch_nlm(const vi_source& src, int X, int Y, int Z, int s, float h, double bias, int rician, float* out, uint32_t* zeroed,
                         hipStream_t stream) {
  static mud_attr_once once;                   // (one per kernel instance)
  if (int e = vi_allow_lds("mud_volume_denoise_nlm", once, (const void*)k_vd_nlm<T, R>, VD_MAX_LDS - 64)) return e;
  const int staged = vd_staged_floats(s, R);
  const size_t bytes = sizeof(float) * ((size_t)staged + 2 * vd_plane<R>::FLOATS);
  hipLaunchKernelGGL((k_vd_nlm<T, R>), vi_tile_grid(X, Y, Z), dim3(VI_THREADS), bytes, stream, src, X, Y, Z, s, staged, h, bias, rician, out, zeroed);
  return MUD_OK;
}

extern "C" int mud_volume_denoise_nlm(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, int search, int patch,
                                      double sigma, double beta, int rician, float* out, uint32_t* zeroed, void* stream) {
  if (int e = vi_check_volume("mud_volume_denoise_nlm", vol, datatype, X, Y, Z)) return e;
  MUD_REQUIRE(out != nullptr && zeroed != nullptr, "mud_volume_denoise_nlm: null pointer");
  MUD_REQUIRE((const void*)out != vol, "mud_volume_denoise_nlm: out must be a buffer of its own");
  MUD_REQUIRE(vi_aligned(out, 4) && vi_aligned(zeroed, 4), "mud_volume_denoise_nlm: out and zeroed must be 4-byte aligned");
  MUD_REQUIRE(search >= 1 && search <= VD_MAX_SEARCH, "mud_volume_denoise_nlm: search radius %d is not in [1, %d]", search, VD_MAX_SEARCH);
  MUD_REQUIRE(patch >= 1 && patch <= VD_MAX_PATCH, "mud_volume_denoise_nlm: patch radius %d is not in [1, %d]", patch, VD_MAX_PATCH);
  MUD_REQUIRE(sigma > 0.0 && sigma - sigma == 0.0 && beta > 0.0 && beta - beta == 0.0, "mud_volume_denoise_nlm: sigma and beta must be finite and > 0 (%g, %g)",
              sigma, beta);
  if (int e = vi_check_tiled("mud_volume_denoise_nlm", X, Y, Z)) return e;
  const size_t bytes = sizeof(float) * ((size_t)vd_staged_floats(search, patch) +
                                        2 * (size_t)(patch == 1 ? vd_plane<1>::FLOATS : vd_plane<2>::FLOATS));
  MUD_REQUIRE(bytes <= VD_MAX_LDS - 64, "mud_volume_denoise_nlm: a halo of %d + %d voxels needs %zu B of LDS, more than %d", search, patch, bytes,
              VD_MAX_LDS - 64);
  double hh = 2.0 * beta;
  hh = hh * sigma;
  hh = hh * sigma;
  double bias = 2.0 * sigma;
  bias = bias * sigma;
  const float h = (float)hh;
  MUD_REQUIRE(h > 0.0f && h - h == 0.0f, "mud_volume_denoise_nlm: 2 beta sigma^2 = %g is not a positive fp32", hh);
  hipStream_t s = (hipStream_t)stream;
  if (int e = vi_clear("mud_volume_denoise_nlm", zeroed, sizeof(uint32_t), s)) return e;
  const vi_source src = vi_source_of(vol, datatype, slope, inter);
  int e = MUD_OK;
  if (patch == 1) {
    VI_DISPATCH(datatype, e = (vd_launch_nlm<T, 1>(src, X, Y, Z, search, h, bias, rician != 0, out, zeroed, s)));
  } else {
    VI_DISPATCH(datatype, e = (vd_launch_nlm<T, 2>(src, X, Y, Z, search, h, bias, rician != 0, out, zeroed, s)));
  }
  if (e) return e;
  MUD_CHECK_LAUNCH("mud_volume_denoise_nlm");
  return MUD_OK;
}
