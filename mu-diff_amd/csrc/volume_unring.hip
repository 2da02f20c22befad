// Removal of truncation (Gibbs) ringing from the volume pipeline's inputs (--unring; include/mudiff_hip.h: mud_volume_unring_*;
// mudiff_hip.volume_unring; DESIGN.md section 5.30 holds the definition both this file and tests/volume_unring_ref.py implement).
//
// Every operator of the definition is a circulant along one storage axis of at most VU_MAX_N voxels, so every kernel here is a "line
// kernel": a workgroup owns a tile of TL whole lines along that axis, neighbours along the faster of the other two axes (global loads
// and stores run along the line when the line is the x axis and across the tile's lines otherwise: coalesced either way), stages them in
// LDS once and writes every voxel of them once.  A workgroup that owns whole lines may work in place.
//
// The directional filter (1 - 3): Ix = I filtered by Gx(kx, ky) per slice.  (1) the dense DFT along x of every line, kx <= nx/2 only
// (real input), its real part left in `ix` and its imaginary part in `iy` AT THE VOXEL (kx, y): the two outputs are the workspace.  (2) per
// (kx, slice) the circular convolution along y with the real kernel g_kx = the inverse transform of Gx(kx, .), in place.  (3) the inverse
// DFT along x of every line from its own nx/2 + 1 bins, Ix to `ix` and Iy = I - Ix to `iy`.  The tables (twiddles, g) come from the host
// in fp64 and the three sums run in fp64, so that Ix is the definition's rounded to fp32 but for the fp32 spectrum in between (measured:
// DESIGN.md section 5.30): the shift bank scores near ties, which an Ix that is off by a few ulp decides differently.  (1) - (3) take
// 2.8 of the stage's 11 ms on a 240 x 240 x 155 volume.
//
// The shift bank (4): per line and shift s_j the line y_s = D_s (*) x (a [lines x n] . [n x n] product per shift that is never stored
// outside LDS), its local total variation left and right of every voxel, and per voxel the running (smallest TV, re-interpolated value,
// j).  A thread forms a 4 lines x 4 positions block of y_s from b128 LDS reads - the row of D_s is held twice over, so that its index
// l - m never wraps, and slides through registers, one new b128 per four m - and writes it, with a wrapped halo of b + 1 voxels, to one of
// two y planes: one barrier per shift.  The TV pass then gives each thread 16 voxels with consecutive lanes on consecutive voxels.
//
// Numerics: every sum is a chain in index order (fp64 fma in the filter, fp32 fmaf in the shift bank, everything else uncontracted), all
// counters are integers: two runs give the same bits.
#include "volume_common.h"

#define VU_MAX_N 512
#define VU_MAX_SHIFTS 32
#define VU_MAX_WINDOW 8
#define VU_MAX_TL 64                           // lines per workgroup of the shift bank, at most
#define VU_OUT 16                              // voxels per thread in its TV pass: TL * n <= VU_OUT * VI_THREADS
#define VU_DFT_TL 8                            // lines per workgroup of the two transforms (fp64 in LDS)
#define VU_MAX_LDS (64 * 1024)

extern __shared__ __attribute__((aligned(16))) float vu_lds[];
#define vu_lds64 ((double*)vu_lds)

// ---- lines along one storage axis, in tiles ---------------------------------------------------------------------------------------------
struct vu_geom {
  int n;                                       // voxels per line
  int nu, nv;                                  // lines: nu along the faster of the other two axes, nv along the slower
  int TL, tiles_u;                             // a tile: TL neighbours along u
  int64_t sa, su, sv;                          // strides in voxels: along the line, along u, along v
};

static vu_geom vu_geom_of(const int dims[3], int axis, int u, int v, int TL) {
  const int64_t stride[3] = {1, dims[0], (int64_t)dims[0] * dims[1]};
  vu_geom g;
  g.n = dims[axis], g.nu = dims[u], g.nv = dims[v], g.TL = TL, g.tiles_u = (int)mud_cdiv(dims[u], TL);
  g.sa = stride[axis], g.su = stride[u], g.sv = stride[v];
  return g;
}

static inline unsigned vu_tiles(const vu_geom& g) { return (unsigned)((int64_t)g.nv * g.tiles_u); }

__device__ __forceinline__ void vu_tile(const vu_geom& g, int& u0, int& v) {
  v = (int)(blockIdx.x / (unsigned)g.tiles_u);
  u0 = (int)(blockIdx.x - (unsigned)v * (unsigned)g.tiles_u) * g.TL;
}

// entry idx of a pass over len entries of each of the tile's lines -> (line of the tile, entry): along the line when that is contiguous in
// memory, across the lines otherwise
__device__ __forceinline__ void vu_split(const vu_geom& g, int idx, int len, int& lt, int& i) {
  if (g.sa == 1) {
    lt = idx / len, i = idx - lt * len;
  } else {
    i = idx / g.TL, lt = idx - i * g.TL;
  }
}

__device__ __forceinline__ int64_t vu_at(const vu_geom& g, int u, int v, int i) { return u * g.su + v * g.sv + i * g.sa; }

template <typename T>                          // a stored voxel, a non-finite one read as 0 and counted
__device__ __forceinline__ float vu_voxel(const vi_source& src, int64_t i, uint32_t& bad) {
  const float v = vi_at<T>(src, i);
  if (vc_finite(v)) return v;
  bad += 1;
  return 0.0f;
}

// ---- 1: the half spectrum along x of every line: re -> ix, im -> iy at the voxel (kx, .) -------------------------------------------------
template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_vu_dft_forward(vi_source src, vu_geom g, const double* __restrict__ twiddle, float* __restrict__ ix,
                                                               float* __restrict__ iy, uint32_t* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  __shared__ uint32_t nbad;
  const int n = g.n, nk = n / 2 + 1, RS = n | 1;
  double* xs = vu_lds64;                       // [TL][RS]
  double* tw = vu_lds64 + g.TL * RS;           // [n] (cos, -sin)
  int u0, v;
  vu_tile(g, u0, v);
  vc_hist_clear(&nbad, 1);
  uint32_t bad = 0;
  for (int idx = threadIdx.x; idx < g.TL * n; idx += VI_THREADS) {
    int lt, i;
    vu_split(g, idx, n, lt, i);
    xs[lt * RS + i] = u0 + lt < g.nu ? (double)vu_voxel<T>(src, vu_at(g, u0 + lt, v, i), bad) : 0.0;
  }
  for (int i = threadIdx.x; i < 2 * n; i += VI_THREADS) tw[i] = twiddle[i];
  if (bad) atomicAdd(&nbad, bad);
  __syncthreads();
  for (int o = threadIdx.x; o < g.TL * nk; o += VI_THREADS) {
    int lt, k;
    vu_split(g, o, nk, lt, k);
    if (u0 + lt >= g.nu) continue;
    const double* x = xs + lt * RS;
    double re = 0.0, im = 0.0;
    int m = 0;                                 // k * l mod n
    for (int l = 0; l < n; ++l) {
      re = fma(x[l], tw[2 * m], re);
      im = fma(x[l], tw[2 * m + 1], im);
      m += k;
      m = m >= n ? m - n : m;
    }
    const int64_t at = vu_at(g, u0 + lt, v, k);
    ix[at] = (float)re, iy[at] = (float)im;
  }
  vc_hist_merge(&nbad, 1, nonfinite);
}

// ---- 2: per (kx, slice) the circular convolution along y of the complex line with the real kernel g_kx, in place -------------------------
// g: the lines along y; the x axis is its u or its v (x_is_u), and only the lines with kx <= nx/2 exist for it (nu or nv is nx/2 + 1)
__global__ __launch_bounds__(VI_THREADS) void k_vu_direction(vu_geom g, int x_is_u, const double* __restrict__ kernel, float* __restrict__ ix,
                                                             float* __restrict__ iy) {
#pragma clang fp contract(off)
  const int n = g.n, RS = n | 1;
  double* zre = vu_lds64;                      // [TL][RS]
  double* zim = zre + g.TL * RS;               // [TL][RS]
  double* g2 = zim + g.TL * RS;                // [TL][2 n]: g2[i] = g_kx[i mod n]
  int u0, v;
  vu_tile(g, u0, v);
  for (int idx = threadIdx.x; idx < g.TL * n; idx += VI_THREADS) {
    int lt, i;
    vu_split(g, idx, n, lt, i);
    const bool have = u0 + lt < g.nu;
    const int64_t at = have ? vu_at(g, u0 + lt, v, i) : 0;
    zre[lt * RS + i] = have ? (double)ix[at] : 0.0;
    zim[lt * RS + i] = have ? (double)iy[at] : 0.0;
    const int kx = x_is_u ? u0 + lt : v;
    const double w = have ? kernel[(int64_t)kx * n + i] : 0.0;
    g2[lt * 2 * n + i] = w, g2[lt * 2 * n + n + i] = w;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < g.TL * n; o += VI_THREADS) {
    const int lt = o / n, r = o - lt * n;      // consecutive lanes on consecutive r: the kernel is read without bank conflicts, z broadcast
    if (u0 + lt >= g.nu) continue;
    const double* a = zre + lt * RS;
    const double* b = zim + lt * RS;
    const double* w = g2 + lt * 2 * n + r + n; // w[-m] = g_kx[(r - m) mod n]
    double re = 0.0, im = 0.0;
    for (int m = 0; m < n; ++m) {
      re = fma(a[m], w[-m], re);
      im = fma(b[m], w[-m], im);
    }
    const int64_t at = vu_at(g, u0 + lt, v, r);
    ix[at] = (float)re, iy[at] = (float)im;
  }
}

// ---- 3: the inverse transform along x of every line from its nx/2 + 1 bins: Ix -> ix, Iy = I - Ix -> iy -----------------------------------
template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_vu_dft_inverse(vi_source src, vu_geom g, const double* __restrict__ twiddle, float* __restrict__ ix,
                                                               float* __restrict__ iy) {
#pragma clang fp contract(off)
  const int n = g.n, nk = n / 2 + 1, RS = nk | 1;
  double* fre = vu_lds64;                      // [TL][RS], each bin times its weight: 1/n for kx = 0 and 2 kx = n, 2/n otherwise
  double* fim = fre + g.TL * RS;
  double* tw = fim + g.TL * RS;
  int u0, v;
  vu_tile(g, u0, v);
  const double w1 = 1.0 / (double)n, w2 = 2.0 / (double)n;
  for (int idx = threadIdx.x; idx < g.TL * nk; idx += VI_THREADS) {
    int lt, k;
    vu_split(g, idx, nk, lt, k);
    const bool have = u0 + lt < g.nu;
    const int64_t at = have ? vu_at(g, u0 + lt, v, k) : 0;
    const double w = (k == 0 || 2 * k == n) ? w1 : w2;
    fre[lt * RS + k] = have ? (double)ix[at] * w : 0.0;
    fim[lt * RS + k] = have ? (double)iy[at] * w : 0.0;
  }
  for (int i = threadIdx.x; i < 2 * n; i += VI_THREADS) tw[i] = twiddle[i];
  __syncthreads();
  uint32_t unused = 0;
  for (int o = threadIdx.x; o < g.TL * n; o += VI_THREADS) {
    int lt, l;
    vu_split(g, o, n, lt, l);
    if (u0 + lt >= g.nu) continue;
    const double* a = fre + lt * RS;
    const double* b = fim + lt * RS;
    double acc = 0.0;
    int m = 0;                                 // k * l mod n
    for (int k = 0; k < nk; ++k) {             // Re(F_k exp(+i t)) = re cos t - im sin t, the table holding (cos t, -sin t)
      acc = fma(a[k], tw[2 * m], acc);
      acc = fma(b[k], tw[2 * m + 1], acc);
      m += l;
      m = m >= n ? m - n : m;
    }
    const int64_t at = vu_at(g, u0 + lt, v, l);
    const float value = vu_voxel<T>(src, at, unused);
    const float mine = (float)acc;
    ix[at] = mine, iy[at] = value - mine;
  }
}

// ---- 4: the shift bank ---------------------------------------------------------------------------------------------------------------------
// LDS, in floats: xs [TL][NP] the lines, zero-padded to NP = n rounded up to 4; ys [2][TL][YS] the shifted lines of the current and the
// previous shift with H = b + 1 wrapped voxels on either side (YS = n + 2 H); d2 [2][2 NP + 8] the rows of D for the current and the
// next shift, d2[i] = D_s[(i - NP - 4) mod n]
static inline int vu_bank_lines(int n) {       // TL: 4 lines per thread-block of positions, at most one block per thread
  const int chunks = (n + 3) / 4, groups = VI_THREADS / chunks;
  return 4 * (groups < VU_MAX_TL / 4 ? groups : VU_MAX_TL / 4);
}
static inline size_t vu_bank_floats(int n, int b, int TL) {
  const int NP = (n + 3) / 4 * 4;
  return (size_t)TL * NP + 2 * (size_t)TL * (n + 2 * (b + 1)) + 2 * (size_t)(2 * NP + 8);
}

__global__ __launch_bounds__(VI_THREADS) void k_vu_lines(const float* in, vu_geom g, int N, int a, int b, const float* __restrict__ table, float* out,
                                                         int accumulate, int8_t* __restrict__ jmap, unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
  const int n = g.n, TL = g.TL, NP = (n + 3) / 4 * 4, H = b + 1, YS = n + 2 * H, D2N = 2 * NP + 8, OFF = NP + 4, K = 2 * N + 1;
  float* xs = vu_lds;
  float* ys = xs + TL * NP;
  float* d2 = ys + 2 * TL * YS;
  const int tid = threadIdx.x;
  int u0, v;
  vu_tile(g, u0, v);
  for (int idx = tid; idx < TL * n; idx += VI_THREADS) {
    int lt, i;
    vu_split(g, idx, n, lt, i);
    xs[lt * NP + i] = u0 + lt < g.nu ? in[vu_at(g, u0 + lt, v, i)] : 0.0f;
  }
  for (int idx = tid; idx < TL * (NP - n); idx += VI_THREADS) {
    const int lt = idx / (NP - n), i = idx - lt * (NP - n);
    xs[lt * NP + n + i] = 0.0f;
  }
  // the product: this thread's block of 4 lines x 4 positions
  const int chunks = NP / 4;
  const bool works = tid < chunks * (TL / 4);
  const int line0 = works ? 4 * (tid / chunks) : 0, l0 = works ? 4 * (tid % chunks) : 0;
  // the TV pass: voxel o = tid + k * VI_THREADS of the tile, l fastest; where its y sits in a y plane, -1 beyond the tile
  int pos[VU_OUT], jbest[VU_OUT];
  float best[VU_OUT], cand[VU_OUT];
#pragma unroll
  for (int k = 0; k < VU_OUT; ++k) {
    const int o = tid + k * VI_THREADS, lt = o / n;
    pos[k] = o < TL * n ? lt * YS + H + (o - lt * n) : -1;
    jbest[k] = 0, best[k] = 0.0f, cand[k] = 0.0f;
  }
  __syncthreads();
  for (int j = 0; j < K; ++j) {
    const int q = j & 1;
    if (works) {
      float acc[4][4];
      if (j == 0) {                            // y_0 = x, not through the sum
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const f32x4 xv = *(const f32x4*)(xs + (line0 + r) * NP + l0);
#pragma unroll
          for (int p = 0; p < 4; ++p) acc[r][p] = xv[p];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int p = 0; p < 4; ++p) acc[r][p] = 0.0f;
        const f32x4* row = (const f32x4*)(d2 + q * D2N);
        f32x4 hi = row[(l0 + OFF) / 4];
        for (int m0 = 0; m0 < NP; m0 += 4) {   // w[i] = d2[l0 - m0 + OFF - 4 + i]: D_s[(l - m) mod n] is w[4 + (l - l0) - (m - m0)]
          const f32x4 lo = row[(l0 - m0 + OFF) / 4 - 1];
          const float w[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const f32x4 xv = *(const f32x4*)(xs + (line0 + r) * NP + m0);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int p = 0; p < 4; ++p) acc[r][p] = fmaf(xv[e], w[4 + p - e], acc[r][p]);
          }
          hi = lo;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float* y = ys + (q * TL + line0 + r) * YS + H;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int l = l0 + p;
          if (l >= n) continue;
          y[l] = acc[r][p];
          if (l < H) y[n + l] = acc[r][p];
          if (l >= n - H) y[l - n] = acc[r][p];
        }
      }
    }
    if (j + 1 < K) {                           // the row of the next shift
      float* next = d2 + (q ^ 1) * D2N;
      const float* D = table + (int64_t)(j + 1) * n;
      for (int i = tid; i < D2N; i += VI_THREADS) {
        int m = (i - OFF) % n;
        m = m < 0 ? m + n : m;
        next[i] = D[m];
      }
    }
    __syncthreads();
    const float* plane = ys + q * TL * YS;
    const int mag = j <= N ? j : j - N;
    const float s = (float)((double)mag / (double)K);
    const int toward = j <= N ? -1 : 1;        // s > 0: y[l - 1]; s < 0: y[l + 1]
#pragma unroll
    for (int k = 0; k < VU_OUT; ++k) {
      if (pos[k] < 0) continue;
      const float* y = plane + pos[k];
      float tvl = 0.0f, tvr = 0.0f;
      for (int t = a; t <= b; ++t) {
        tvl = tvl + fabsf(y[-t] - y[-t - 1]);
        tvr = tvr + fabsf(y[t + 1] - y[t]);
      }
      const float tv = tvl < tvr ? tvl : tvr;
      if (j == 0) {
        best[k] = tv, cand[k] = y[0];
      } else if (tv < best[k]) {               // strict: a tie keeps the earlier shift
        const float a1 = y[0];
        float step = y[toward] - a1;
        step = s * step;
        best[k] = tv, cand[k] = a1 + step, jbest[k] = j;
      }
    }
  }
  // the result through LDS, so that it leaves as the lines came: values in xs (the products are done), j in the y plane nobody reads any more
  int* js = (int*)(ys + TL * YS);              // plane 1: K is odd, the last shift used plane 0
  uint32_t moved = 0, total = 0;
#pragma unroll
  for (int k = 0; k < VU_OUT; ++k) {
    if (pos[k] < 0) continue;
    const int o = tid + k * VI_THREADS, lt = o / n, l = o - lt * n;
    xs[lt * NP + l] = cand[k];
    js[lt * YS + l] = jbest[k];
    if (u0 + lt < g.nu) {
      moved += jbest[k] != 0;
      total += (uint32_t)(jbest[k] <= N ? jbest[k] : jbest[k] - N);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) moved += __shfl_xor(moved, o, 64), total += __shfl_xor(total, o, 64);
  if ((tid & 63) == 0) {
    if (moved) atomicAdd(&counters[0], (unsigned long long)moved);
    if (total) atomicAdd(&counters[1], (unsigned long long)total);
  }
  __syncthreads();
  for (int idx = tid; idx < TL * n; idx += VI_THREADS) {
    int lt, i;
    vu_split(g, idx, n, lt, i);
    if (u0 + lt >= g.nu) continue;
    const int64_t at = vu_at(g, u0 + lt, v, i);
    const float value = xs[lt * NP + i];
    out[at] = accumulate ? out[at] + value : value;
    if (jmap) jmap[at] = (int8_t)js[lt * YS + i];
  }
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------
static int vu_check_axes(const char* who, int a, int b) {
  MUD_REQUIRE(a >= 0 && a <= 2 && b >= 0 && b <= 2 && a != b, "%s: two distinct storage axes in [0, 2], got %d and %d", who, a, b);
  return MUD_OK;
}

extern "C" int mud_volume_unring_filter(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, int axis_x, int axis_y,
                                        const double* twiddle, const double* kernel, float* ix, float* iy, uint32_t* nonfinite, void* stream) {
  const char* who = "mud_volume_unring_filter";
  if (int e = vi_check_volume(who, vol, datatype, X, Y, Z)) return e;
  if (int e = vu_check_axes(who, axis_x, axis_y)) return e;
  MUD_REQUIRE(twiddle != nullptr && kernel != nullptr && ix != nullptr && iy != nullptr && nonfinite != nullptr, "%s: null pointer", who);
  MUD_REQUIRE(vi_aligned(twiddle, 8) && vi_aligned(kernel, 8) && vi_aligned(ix, 4) && vi_aligned(iy, 4) && vi_aligned(nonfinite, 4),
              "%s: the tables must be 8-byte, ix, iy and nonfinite 4-byte aligned", who);
  MUD_REQUIRE(ix != iy && (const void*)ix != vol && (const void*)iy != vol, "%s: ix and iy must be buffers of their own", who);
  const int dims[3] = {X, Y, Z}, normal = 3 - axis_x - axis_y;
  const int nx = dims[axis_x], ny = dims[axis_y];
  MUD_REQUIRE(nx >= 2 && nx <= VU_MAX_N && ny >= 2 && ny <= VU_MAX_N, "%s: the in-plane axes must have 2 to %d voxels, got %d and %d", who, VU_MAX_N, nx,
              ny);
  hipStream_t s = (hipStream_t)stream;
  if (int e = vi_clear(who, nonfinite, sizeof(uint32_t), s)) return e;
  const vi_source src = vi_source_of(vol, datatype, slope, inter);
  // the lines along x: u the faster of the other two axes
  const vu_geom gx = vu_geom_of(dims, axis_x, axis_y < normal ? axis_y : normal, axis_y < normal ? normal : axis_y, VU_DFT_TL);
  const size_t fwd = sizeof(double) * ((size_t)VU_DFT_TL * (nx | 1) + 2 * (size_t)nx);
  const size_t inv = sizeof(double) * (2 * (size_t)VU_DFT_TL * ((nx / 2 + 1) | 1) + 2 * (size_t)nx);
  // the lines along y at kx <= nx/2
  const int TLy = ny > VU_MAX_N / 2 ? 2 : 4, x_is_u = axis_x < normal;
  int half[3] = {X, Y, Z};
  half[axis_x] = nx / 2 + 1;
  vu_geom gy = vu_geom_of(half, axis_y, x_is_u ? axis_x : normal, x_is_u ? normal : axis_x, TLy);
  const vu_geom whole = vu_geom_of(dims, axis_y, x_is_u ? axis_x : normal, x_is_u ? normal : axis_x, TLy);
  gy.sa = whole.sa, gy.su = whole.su, gy.sv = whole.sv;      // (the strides of the whole volume)
  const size_t dir = sizeof(double) * ((size_t)TLy * (2 * (size_t)(ny | 1) + 2 * (size_t)ny));
  MUD_REQUIRE(fwd <= VU_MAX_LDS && inv <= VU_MAX_LDS && dir <= VU_MAX_LDS, "%s: %zu / %zu / %zu B of LDS, more than %d", who, fwd, dir, inv, VU_MAX_LDS);
  VI_DISPATCH(datatype, hipLaunchKernelGGL(k_vu_dft_forward<T>, dim3(vu_tiles(gx)), dim3(VI_THREADS), fwd, s, src, gx, twiddle, ix, iy, nonfinite));
  MUD_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(k_vu_direction, dim3(vu_tiles(gy)), dim3(VI_THREADS), dir, s, gy, x_is_u, kernel, ix, iy);
  MUD_CHECK_LAUNCH(who);
  VI_DISPATCH(datatype, hipLaunchKernelGGL(k_vu_dft_inverse<T>, dim3(vu_tiles(gx)), dim3(VI_THREADS), inv, s, src, gx, twiddle, ix, iy));
  MUD_CHECK_LAUNCH(who);
  return MUD_OK;
}

extern "C" int mud_volume_unring_lines(const float* in, int X, int Y, int Z, int axis, int normal, int shifts, int a, int b, const float* table,
                                       float* out, int accumulate, int8_t* jmap, uint64_t* counters, void* stream) {
  const char* who = "mud_volume_unring_lines";
  if (int e = vi_check_size(who, "volume", X, Y, Z)) return e;
  if (int e = vu_check_axes(who, axis, normal)) return e;
  MUD_REQUIRE(in != nullptr && table != nullptr && out != nullptr && counters != nullptr, "%s: null pointer", who);
  MUD_REQUIRE(vi_aligned(in, 4) && vi_aligned(table, 4) && vi_aligned(out, 4) && vi_aligned(counters, 8), "%s: in, table and out must be 4-byte, counters 8-byte aligned",
              who);
  MUD_REQUIRE(shifts >= 1 && shifts <= VU_MAX_SHIFTS, "%s: %d shifts per side are not in [1, %d]", who, shifts, VU_MAX_SHIFTS);
  MUD_REQUIRE(a >= 1 && a <= b && b <= VU_MAX_WINDOW, "%s: the window %d .. %d is not 1 <= a <= b <= %d", who, a, b, VU_MAX_WINDOW);
  const int dims[3] = {X, Y, Z}, other = 3 - axis - normal;
  const int n = dims[axis];
  MUD_REQUIRE(n >= 2 * b + 2 && n <= VU_MAX_N, "%s: lines of %d voxels are not in [2 b + 2 = %d, %d]", who, n, 2 * b + 2, VU_MAX_N);
  const int TL = vu_bank_lines(n);
  const size_t bytes = sizeof(float) * vu_bank_floats(n, b, TL);
  MUD_REQUIRE(TL >= 4 && (int64_t)TL * n <= VU_OUT * VI_THREADS && bytes <= VU_MAX_LDS, "%s: a tile of %d lines of %d voxels (%zu B of LDS) does not fit", who, TL,
              n, bytes);
  hipStream_t s = (hipStream_t)stream;
  if (int e = vi_clear(who, counters, 2 * sizeof(uint64_t), s)) return e;
  const vu_geom g = vu_geom_of(dims, axis, normal < other ? normal : other, normal < other ? other : normal, TL);
  hipLaunchKernelGGL(k_vu_lines, dim3(vu_tiles(g)), dim3(VI_THREADS), bytes, s, in, g, shifts, a, b, table, out, accumulate != 0, jmap,
                     (unsigned long long*)counters);
  MUD_CHECK_LAUNCH(who);
  return MUD_OK;
}
