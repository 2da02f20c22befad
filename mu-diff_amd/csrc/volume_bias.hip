// N4-style bias-field correction of the volume pipeline's inputs (--bias_correct; include/mudiff_hip.h: mud_volume_bias_*;
// mudiff_hip.volume_bias).
//
// The estimation loop runs on the host; what it evaluates a few hundred times per volume is here: the log image at the sample points
// (every shrink-th voxel per axis), the log image corrected by the current field F with its extremes and its largest change, its
// histogram, the integer sums of the B-spline fit of its residual against the sharpened histogram's table, and at the end the division
// of every voxel by exp(F).  F is a sum of uniform cubic B-spline lattices, level l with 2^l spans per axis; the lattices of all levels
// sit in LDS.  Every fp64 expression below is evaluated in the order of tests/volume_bias_ref.py with contraction off, so that the
// corrected log image, the bins and the integer sums equal the restatement's bit for bit; only logf and exp are the math library's.
// The sums are integers (LDS atomics per workgroup, one global atomic per non-empty entry): the order of arrival cannot show.
#include "volume_common.h"

#define VB_MAX_LEVELS 5                        // 1, 2, 4, 8, 16 spans per axis: (2^l + 3)^3 control points each
#define VB_MAX_BINS 1024
#define VB_MAX_BLOCKS 1024
#define VB_FIT_SAMPLES 2048                    // samples per workgroup of the fit at least: each merges up to 2 m^3 sums

static inline int vb_lattice_doubles(int levels) {
  int n = 0;
  for (int l = 0; l < levels; ++l) n += ((1 << l) + 3) * ((1 << l) + 3) * ((1 << l) + 3);
  return n;
}

// one axis: voxel index i of S, n spans -> the span and the four weights of its control points span .. span + 3
__device__ __forceinline__ int vb_axis(int i, int S, int n, double b[4]) {
#pragma clang fp contract(off)
  double x = ((double)i + 0.5) * (double)n;
  x = x / (double)S;
  double s = floor(x);
  const double top = (double)(n - 1);
  s = s < top ? s : top;
  const double t = x - s;
  const double omt = 1.0 - t, t2 = t * t;
  const double t3 = t2 * t;
  b[0] = ((omt * omt) * omt) / 6.0;
  b[1] = ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0;
  b[2] = (((3.0 * t2 - 3.0 * t3) + 3.0 * t) + 1.0) / 6.0;
  b[3] = t3 / 6.0;
  return (int)s;
}

// F at the voxel (ix, iy, iz): levels in order, then the 4 x 4 x 4 support with x fastest (shared by the corrected image and the apply)
__device__ __forceinline__ double vb_field(const double* lat, int levels, int ix, int iy, int iz, int X, int Y, int Z) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int l = 0; l < levels; ++l) {
    const int n = 1 << l, m = n + 3;
    double bx[4], by[4], bz[4];
    const int sx = vb_axis(ix, X, n, bx), sy = vb_axis(iy, Y, n, by), sz = vb_axis(iz, Z, n, bz);
#pragma unroll
    for (int dz = 0; dz < 4; ++dz)
#pragma unroll
      for (int dy = 0; dy < 4; ++dy) {
        const double* row = lat + ((sz + dz) * m + (sy + dy)) * m + sx;
#pragma unroll
        for (int dx = 0; dx < 4; ++dx) {
          const double w = (bx[dx] * by[dy]) * bz[dz];
          const double term = w * row[dx];
          acc = acc + term;
        }
      }
    lat += m * m * m;
  }
  return acc;
}

struct vb_grid {                               // the sample points: every shrink-th voxel of X x Y x Z
  int X, Y, Z, shrink, nx, ny;
  int64_t n;
};

__device__ __forceinline__ void vb_sample(const vb_grid& g, int64_t i, int& xi, int& yj, int& zk) {
  vi_xyz(i, g.nx, g.ny, xi, yj, zk);
  xi *= g.shrink, yj *= g.shrink, zk *= g.shrink;
}

// ---- 1: u = logf(v) at the sample points, NaN where the sample is masked out (v not finite, or not > 0)
template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_vb_log(vi_source src, vb_grid g, float* __restrict__ u) {
  VI_GRID_STRIDE(i, g.n) {
    int xi, yj, zk;
    vb_sample(g, i, xi, yj, zk);
    const float v = vi_at<T>(src, ((int64_t)zk * g.Y + yj) * g.X + xi);
    u[i] = (vc_finite(v) && v > 0.0f) ? logf(v) : __uint_as_float(0x7fc00000u);
  }
}

// ---- 2: c = float32(double(u) - F), the finite extremes of c and the largest |c - c_old|
extern __shared__ double vb_lds[];

__global__ __launch_bounds__(VI_THREADS) void k_vb_corrected(const float* __restrict__ u, const float* __restrict__ c_old,
                                                             float* __restrict__ c_new, const double* __restrict__ lattices, int levels,
                                                             int nlat, vb_grid g, unsigned long long* __restrict__ stats) {
  __shared__ unsigned long long red[3];
  for (int i = threadIdx.x; i < nlat; i += VI_THREADS) vb_lds[i] = lattices[i];
  if (threadIdx.x == 0) {
    red[0] = 0ull;
    red[1] = 0ull;
    red[2] = ~0ull;
  }
  __syncthreads();
  unsigned long long dmax = 0ull, kmax = 0ull, kmin = ~0ull;
  VI_GRID_STRIDE(i, g.n) {
    const float uv = u[i];
    float c = uv;
    if (uv == uv) {
      int xi, yj, zk;
      vb_sample(g, i, xi, yj, zk);
      c = (float)((double)uv - vb_field(vb_lds, levels, xi, yj, zk, g.X, g.Y, g.Z));
    }
    c_new[i] = c;
    if (vc_finite(c)) {
      const unsigned long long key = vc_key(c);
      kmax = key > kmax ? key : kmax;
      kmin = key < kmin ? key : kmin;
    }
    const double d = fabs((double)c - (double)c_old[i]);
    if (d == d) {                              // (a non-negative double orders as its bits do)
      const unsigned long long bits = (unsigned long long)__double_as_longlong(d);
      dmax = bits > dmax ? bits : dmax;
    }
  }
  atomicMax(&red[0], dmax);
  atomicMax(&red[1], kmax);
  atomicMin(&red[2], kmin);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (red[0]) atomicMax(&stats[0], red[0]);
    if (red[1]) atomicMax(&stats[1], red[1]);
    if (red[2] != ~0ull) atomicMin(&stats[2], red[2]);
  }
}

// ---- 3a: the histogram of the finite c
__global__ __launch_bounds__(VI_THREADS) void k_vb_hist(const float* __restrict__ c, int64_t n, double lo, double scale, int bins,
                                                        uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[VB_MAX_BINS];
  vc_hist_clear(h, bins);
  VI_GRID_STRIDE(i, n) {
    const float v = c[i];
    if (vc_finite(v)) atomicAdd(&h[vc_bin(v, lo, scale, bins)], 1u);
  }
  vc_hist_merge(h, bins, hist);
}

// table(c): linear interpolation between bin centres in fp64, clamped at the ends (bins >= 2)
__device__ __forceinline__ double vb_table_at(float c, const double* table, double lo, double scale, int bins) {
#pragma clang fp contract(off)
  double p = (double)c - lo;
  p = p * scale;
  p = p - 0.5;
  const double top = (double)(bins - 1), last = (double)(bins - 2);
  p = p > 0.0 ? p : 0.0;
  p = p < top ? p : top;
  double fi = floor(p);
  fi = fi < last ? fi : last;
  const int i = (int)fi;
  const double f = p - fi;
  const double step = table[i + 1] - table[i];
  const double up = f * step;
  return table[i] + up;
}

// ---- 3b: the integer sums of one level's fit of r = c - table(c): per finite sample and control point of its 4 x 4 x 4 support,
// delta += llrint(w^3 r / S2 * 2^k), omega += llrint(w^2 * 2^k).  LDS: delta [m^3], omega [m^3] (int64), then the table [bins]
__global__ __launch_bounds__(VI_THREADS) void k_vb_fit(const float* __restrict__ c, const double* __restrict__ table, int bins, double lo,
                                                       double scale, int level, vb_grid g, double two_k,
                                                       unsigned long long* __restrict__ sums) {
#pragma clang fp contract(off)
  const int n = 1 << level, m = n + 3, m3 = m * m * m;
  unsigned long long* acc = (unsigned long long*)vb_lds;
  double* tab = vb_lds + 2 * m3;
  for (int i = threadIdx.x; i < 2 * m3; i += VI_THREADS) acc[i] = 0ull;
  for (int i = threadIdx.x; i < bins; i += VI_THREADS) tab[i] = table[i];
  __syncthreads();
  VI_GRID_STRIDE(i, g.n) {
    const float cv = c[i];
    if (!vc_finite(cv)) continue;
    int xi, yj, zk;
    vb_sample(g, i, xi, yj, zk);
    double bx[4], by[4], bz[4];
    const int sx = vb_axis(xi, g.X, n, bx), sy = vb_axis(yj, g.Y, n, by), sz = vb_axis(zk, g.Z, n, bz);
    const double r = (double)cv - vb_table_at(cv, tab, lo, scale, bins);
    const double qx = ((bx[0] * bx[0] + bx[1] * bx[1]) + bx[2] * bx[2]) + bx[3] * bx[3];
    const double qy = ((by[0] * by[0] + by[1] * by[1]) + by[2] * by[2]) + by[3] * by[3];
    const double qz = ((bz[0] * bz[0] + bz[1] * bz[1]) + bz[2] * bz[2]) + bz[3] * bz[3];
    const double S2 = (qx * qy) * qz;
#pragma unroll
    for (int dz = 0; dz < 4; ++dz)
#pragma unroll
      for (int dy = 0; dy < 4; ++dy) {
        const int row = ((sz + dz) * m + (sy + dy)) * m + sx;
#pragma unroll
        for (int dx = 0; dx < 4; ++dx) {
          const double w = (bx[dx] * by[dy]) * bz[dz];
          const double w2 = w * w;
          double d = w2 * w;
          d = d * r;
          d = d / S2;
          d = d * two_k;
          const double o = w2 * two_k;
          atomicAdd(&acc[row + dx], (unsigned long long)llrint(d));          // (two's complement: the unsigned sum is the signed one)
          atomicAdd(&acc[m3 + row + dx], (unsigned long long)llrint(o));
        }
      }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * m3; i += VI_THREADS) {
    const unsigned long long v = acc[i];
    if (v) atomicAdd(&sums[i], v);
  }
}

// ---- 4: every voxel / exp(F) (or exp(F) itself with `field`), four consecutive voxels per thread, one 16-byte store
__global__ __launch_bounds__(VI_THREADS) void k_vb_apply(vi_source src, const double* __restrict__ lattices, int levels, int nlat, int X, int Y,
                                                         int Z, int64_t n, int field, float* __restrict__ out) {
  for (int i = threadIdx.x; i < nlat; i += VI_THREADS) vb_lds[i] = lattices[i];
  __syncthreads();
  const int64_t quads = (n + 3) / 4;
  VI_GRID_STRIDE(q, quads) {
    float res[4];
    const int64_t base = q * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t i = base + e;
      res[e] = 0.0f;
      if (i >= n) continue;
      int xi, yj, zk;
      vi_xyz(i, X, Y, xi, yj, zk);
      const float v = vc_stored_value(src, i);
      if (!field && !(vc_finite(v) && v != 0.0f)) {          // a zero stays zero, a non-finite voxel passes through
        res[e] = v;
        continue;
      }
      const double ef = exp(vb_field(vb_lds, levels, xi, yj, zk, X, Y, Z));
      res[e] = field ? (float)ef : (float)((double)v / ef);
    }
    if (base + 3 < n) {
      f32x4 o = {res[0], res[1], res[2], res[3]};
      *(f32x4*)(out + base) = o;
    } else {
      for (int e = 0; e < 4 && base + e < n; ++e) out[base + e] = res[e];
    }
  }
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------
static inline int vb_check_grid(const char* who, int X, int Y, int Z, int shrink, vb_grid* g) {
  if (int e = vi_check_size(who, "volume", X, Y, Z)) return e;
  MUD_REQUIRE(shrink > 0, "%s: shrink %d is not positive", who, shrink);
  g->X = X, g->Y = Y, g->Z = Z, g->shrink = shrink;
  g->nx = (int)mud_cdiv(X, shrink), g->ny = (int)mud_cdiv(Y, shrink);
  g->n = (int64_t)g->nx * g->ny * mud_cdiv(Z, shrink);
  return MUD_OK;
}

#define VB_FIELD_LDS_MAX (8722 * 8)                                        // vb_lattice_doubles(VB_MAX_LEVELS) doubles
#define VB_FIT_LDS_MAX (2 * 19 * 19 * 19 * 8 + VB_MAX_BINS * 8)            // level VB_MAX_LEVELS - 1, VB_MAX_BINS bins

extern "C" int mud_volume_bias_log(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, int shrink, float* u,
                                   void* stream) {
  if (int e = vi_check_volume("mud_volume_bias_log", vol, datatype, X, Y, Z)) return e;
  vb_grid g;
  if (int e = vb_check_grid("mud_volume_bias_log", X, Y, Z, shrink, &g)) return e;
  MUD_REQUIRE(u != nullptr, "mud_volume_bias_log: null pointer");
  VI_DISPATCH(datatype, hipLaunchKernelGGL(k_vb_log<T>, dim3(vi_blocks(g.n, VI_THREADS, VB_MAX_BLOCKS)), dim3(VI_THREADS), 0, (hipStream_t)stream,
                                           vi_source_of(vol, datatype, slope, inter), g, u));
  MUD_CHECK_LAUNCH("mud_volume_bias_log");
  return MUD_OK;
}

extern "C" int mud_volume_bias_corrected(const float* u, const float* c_old, float* c_new, const double* lattices, int levels, int X, int Y,
                                         int Z, int shrink, uint64_t* stats, void* stream) {
  vb_grid g;
  if (int e = vb_check_grid("mud_volume_bias_corrected", X, Y, Z, shrink, &g)) return e;
  MUD_REQUIRE(u != nullptr && c_old != nullptr && c_new != nullptr && lattices != nullptr && stats != nullptr,
              "mud_volume_bias_corrected: null pointer");
  MUD_REQUIRE(c_old != c_new && u != c_new, "mud_volume_bias_corrected: c_new must be a buffer of its own");
  MUD_REQUIRE(vi_aligned(stats, 8) && vi_aligned(lattices, 8), "mud_volume_bias_corrected: stats and lattices must be 8-byte aligned");
  MUD_REQUIRE(levels >= 1 && levels <= VB_MAX_LEVELS, "mud_volume_bias_corrected: 1 to %d levels, got %d", VB_MAX_LEVELS, levels);
  hipStream_t s = (hipStream_t)stream;
  static mud_attr_once once;
  if (int e = vi_allow_lds("mud_volume_bias_corrected", once, (const void*)k_vb_corrected, VB_FIELD_LDS_MAX)) return e;
  if (int e = vi_clear("mud_volume_bias_corrected", stats, 16, s)) return e;                  // two maxima from 0,
  if (int e = vi_clear("mud_volume_bias_corrected", stats + 2, 8, s, 0xFF)) return e;         // the minimum from all ones
  const int nlat = vb_lattice_doubles(levels);
  hipLaunchKernelGGL(k_vb_corrected, dim3(vi_blocks(g.n, VI_THREADS, VB_MAX_BLOCKS)), dim3(VI_THREADS), (size_t)nlat * 8, s, u, c_old, c_new, lattices, levels,
                     nlat, g, (unsigned long long*)stats);
  MUD_CHECK_LAUNCH("mud_volume_bias_corrected");
  return MUD_OK;
}

extern "C" int mud_volume_bias_hist(const float* c, int64_t n, double lo, double scale, int bins, uint32_t* hist, void* stream) {
  MUD_REQUIRE(c != nullptr && hist != nullptr, "mud_volume_bias_hist: null pointer");
  MUD_REQUIRE(n > 0 && n < ((int64_t)1 << 31), "mud_volume_bias_hist: bad sample count %lld", (long long)n);
  if (int e = vi_check_bins("mud_volume_bias_hist", lo, scale, bins, 2, VB_MAX_BINS)) return e;
  MUD_REQUIRE(vi_aligned(hist, 4), "mud_volume_bias_hist: hist must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (int e = vi_clear("mud_volume_bias_hist", hist, sizeof(uint32_t) * bins, s)) return e;
  hipLaunchKernelGGL(k_vb_hist, dim3(vi_blocks(n, VI_THREADS, VB_MAX_BLOCKS)), dim3(VI_THREADS), 0, s, c, n, lo, scale, bins, hist);
  MUD_CHECK_LAUNCH("mud_volume_bias_hist");
  return MUD_OK;
}

extern "C" int mud_volume_bias_fit(const float* c, const double* table, int bins, double lo, double scale, int level, int X, int Y, int Z,
                                   int shrink, int k, int64_t* sums, void* stream) {
  vb_grid g;
  if (int e = vb_check_grid("mud_volume_bias_fit", X, Y, Z, shrink, &g)) return e;
  MUD_REQUIRE(c != nullptr && table != nullptr && sums != nullptr, "mud_volume_bias_fit: null pointer");
  if (int e = vi_check_bins("mud_volume_bias_fit", lo, scale, bins, 2, VB_MAX_BINS)) return e;
  MUD_REQUIRE(vi_aligned(sums, 8) && vi_aligned(table, 8), "mud_volume_bias_fit: sums and table must be 8-byte aligned");
  MUD_REQUIRE(level >= 0 && level < VB_MAX_LEVELS, "mud_volume_bias_fit: level %d: a lattice of more than %d spans per axis does not fit in LDS",
              level, 1 << (VB_MAX_LEVELS - 1));
  MUD_REQUIRE(k >= 0 && k <= 62, "mud_volume_bias_fit: k = %d is not in [0, 62]", k);
  hipStream_t s = (hipStream_t)stream;
  static mud_attr_once once;
  if (int e = vi_allow_lds("mud_volume_bias_fit", once, (const void*)k_vb_fit, VB_FIT_LDS_MAX)) return e;
  const int m = (1 << level) + 3, m3 = m * m * m;
  if (int e = vi_clear("mud_volume_bias_fit", sums, sizeof(int64_t) * 2 * m3, s)) return e;
  hipLaunchKernelGGL(k_vb_fit, dim3(vi_blocks(g.n, VB_FIT_SAMPLES, VB_MAX_BLOCKS)), dim3(VI_THREADS), (size_t)(2 * m3 + bins) * 8, s, c, table, bins, lo, scale,
                     level, g, ldexp(1.0, k), (unsigned long long*)sums);
  MUD_CHECK_LAUNCH("mud_volume_bias_fit");
  return MUD_OK;
}

extern "C" int mud_volume_bias_apply(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, const double* lattices,
                                     int levels, int field, float* out, void* stream) {
  if (int e = vi_check_volume("mud_volume_bias_apply", vol, datatype, X, Y, Z)) return e;
  MUD_REQUIRE(lattices != nullptr && out != nullptr, "mud_volume_bias_apply: null pointer");
  MUD_REQUIRE(mud_aligned16(out) && vi_aligned(lattices, 8), "mud_volume_bias_apply: out must be 16-byte, lattices 8-byte aligned");
  MUD_REQUIRE((const void*)out != vol, "mud_volume_bias_apply: out must be a buffer of its own");
  MUD_REQUIRE(levels >= 1 && levels <= VB_MAX_LEVELS, "mud_volume_bias_apply: 1 to %d levels, got %d", VB_MAX_LEVELS, levels);
  static mud_attr_once once;
  if (int e = vi_allow_lds("mud_volume_bias_apply", once, (const void*)k_vb_apply, VB_FIELD_LDS_MAX)) return e;
  const int64_t n = (int64_t)X * Y * Z;
  const int nlat = vb_lattice_doubles(levels);
  hipLaunchKernelGGL(k_vb_apply, dim3(vi_blocks(mud_cdiv(n, 4), VI_THREADS, VB_MAX_BLOCKS)), dim3(VI_THREADS), (size_t)nlat * 8, (hipStream_t)stream,
                     vi_source_of(vol, datatype, slope, inter), lattices, levels, nlat, X, Y, Z, n, field != 0, out);
  MUD_CHECK_LAUNCH("mud_volume_bias_apply");
  return MUD_OK;
}
