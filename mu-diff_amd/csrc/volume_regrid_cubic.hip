// Cubic B-spline resampling of the volume pipeline (--regrid_interp cubic; include/mudiff_hip.h: mud_volume_bspline_coeffs,
// mud_volume_regrid_cubic; mudiff_hip.volume_regrid).
//
// Two steps.  mud_volume_bspline_coeffs turns the stored volume into the fp64 coefficients c of the cubic B-spline that interpolates
// it under mirror (whole-sample symmetric) boundaries: one recursive filter per line, along x, then y, then z, with the single pole
// z1 = sqrt(3) - 2.  Per line s[0..N-1] (N >= 2; a line of one voxel is its own coefficient), every product and sum rounded separately:
//     g[i]    = 6 s[i]
//     c+[0]   = (sum over k = 0 .. 2N-3 of z1^k g[m(k)]) / (1 - z1^(2N-2)),  m(k) = k for k <= N-1, else 2N-2-k; the sum in increasing k,
//               the power kept as a running product
//     c+[i]   = g[i] + z1 c+[i-1]                                             (causal, i = 1 .. N-1)
//     c[N-1]  = (z1 / (z1 z1 - 1)) (c+[N-1] + z1 c+[N-2])
//     c[i]    = z1 (c[i+1] - c+[i])                                           (anti-causal, i = N-2 .. 0)
// mud_volume_regrid_cubic then gathers the 4 x 4 x 4 coefficients around every output voxel's source coordinate.
//
// The layout of the recursion.  The y and z passes work in place on the coefficients, one thread per line, adjacent threads on adjacent
// x (for z: adjacent x + SX y), so that every load and store of a step of the recursion is one run of consecutive addresses.  The x
// pass cannot do that - adjacent lines are SX elements apart - so a workgroup takes BS_ROWS adjacent lines and moves along them in
// chunks of BS_COLS columns: all 256 threads copy a chunk between global memory and LDS in runs of BS_COLS consecutive elements per
// line, then the first wave walks it, one thread per line, in LDS rows padded by one double (lane t reads the 64-bit word 33 t + c:
// the 32 lanes an LDS cycle serves touch 32 different bank pairs).  A line is swept four times - forward and backward for the sum of
// c+[0], forward for c+, backward for c - and never staged whole: no axis has a maximum length.
// No floating-point atomics and no order that depends on the launch: the same bits on every run.
#include <cmath>
#include "volume_common.h"

#define BS_ROWS 64                             // lines per workgroup of the x pass: one per lane of the wave that runs the recursion
#define BS_COLS 32                             // columns per chunk
#define BS_LD (BS_COLS + 1)                    // the padded LDS row

struct bs_line_state {                         // what a line carries from sweep to sweep
  double a, zk;                                // the running sum of c+[0] and z1^k
  double last, before;                         // c+ of the newest and the second newest position, then c of the newest
};

// one term of the sum of c+[0]
__device__ __forceinline__ void bs_sum_step(bs_line_state& st, double g, double z) {
#pragma clang fp contract(off)
  const double term = st.zk * g;
  st.a = st.a + term;
  st.zk = st.zk * z;
}

__device__ __forceinline__ double bs_causal_first(const bs_line_state& st) {
#pragma clang fp contract(off)
  const double den = 1.0 - st.zk;
  return st.a / den;
}

__device__ __forceinline__ double bs_causal_step(double g, double prev, double z) {
#pragma clang fp contract(off)
  const double t = z * prev;
  return g + t;
}

// c[N-1] from c+[N-1] (last) and c+[N-2] (before)
__device__ __forceinline__ double bs_anticausal_first(double last, double before, double z) {
#pragma clang fp contract(off)
  const double zz = z * z;
  const double den = zz - 1.0;
  const double gain = z / den;
  const double t = z * before;
  const double sum = last + t;
  return gain * sum;
}

__device__ __forceinline__ double bs_anticausal_step(double next, double cplus, double z) {
#pragma clang fp contract(off)
  const double d = next - cplus;
  return z * d;
}

__device__ __forceinline__ double bs_times6(double s) {
#pragma clang fp contract(off)
  return 6.0 * s;
}

// ---- the x pass: stored voxels -> coefficients along x ---------------------------------------------------------------------------------
// the chunk of columns c0 .. c0 + nc - 1 of the workgroup's lines: f(row, column) of every element, lanes along the columns
template <typename F>
__device__ __forceinline__ void bs_chunk(int nrows, int nc, F f) {
  for (int idx = threadIdx.x; idx < BS_ROWS * BS_COLS; idx += VI_THREADS) {
    const int r = idx / BS_COLS, c = idx - r * BS_COLS;
    if (r < nrows && c < nc) f(r, c);
  }
}

template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_bs_x(vi_source src, int SX, int64_t nlines, double z, double* coeffs,
                                                     uint32_t* __restrict__ nonfinite) {
  __shared__ double tile[BS_ROWS][BS_LD];
  __shared__ uint32_t s_bad;
  vc_hist_clear(&s_bad, 1);
  const int64_t l0 = (int64_t)blockIdx.x * BS_ROWS;
  const int nrows = (int)(nlines - l0 < BS_ROWS ? nlines - l0 : BS_ROWS);
  const int64_t base = l0 * SX;
  const int row = threadIdx.x;                 // the line of a thread of the first wave
  const bool walks = row < nrows;              // (nrows <= BS_ROWS = 64: the first wave)
  uint32_t bad = 0;
  // g = 6 s of a chunk into the tile (s alone for a line of one voxel); the non-finite voxels are counted by the sweep that asks
  auto load_source = [&](int c0, int nc, bool count, bool times6) {
    bs_chunk(nrows, nc, [&](int r, int c) {
      const float v = vi_at<T>(src, base + (int64_t)r * SX + c0 + c);
      const bool ok = vc_finite(v);
      if (count && !ok) ++bad;
      const double s = ok ? (double)v : 0.0;
      tile[r][c] = times6 ? bs_times6(s) : s;
    });
  };
  auto store_coeffs = [&](int c0, int nc) {
    bs_chunk(nrows, nc, [&](int r, int c) { coeffs[base + (int64_t)r * SX + c0 + c] = tile[r][c]; });
  };
  if (SX == 1) {                               // c = s
    load_source(0, 1, true, false);
    __syncthreads();
    store_coeffs(0, 1);
  } else {
    const int last_c0 = ((SX - 1) / BS_COLS) * BS_COLS;
    bs_line_state st = {0.0, 1.0, 0.0, 0.0};
    for (int c0 = 0; c0 < SX; c0 += BS_COLS) {                       // k = 0 .. N-1: positions 0 .. N-1
      const int nc = min(BS_COLS, SX - c0);
      load_source(c0, nc, false, true);
      __syncthreads();
      if (walks)
        for (int c = 0; c < nc; ++c) bs_sum_step(st, tile[row][c], z);
      __syncthreads();
    }
    for (int c0 = last_c0; c0 >= 0; c0 -= BS_COLS) {                 // k = N .. 2N-3: positions N-2 .. 1
      const int nc = min(BS_COLS, SX - c0);
      load_source(c0, nc, false, true);
      __syncthreads();
      if (walks)
        for (int c = nc - 1; c >= 0; --c) {
          const int i = c0 + c;
          if (i >= 1 && i <= SX - 2) bs_sum_step(st, tile[row][c], z);
        }
      __syncthreads();
    }
    for (int c0 = 0; c0 < SX; c0 += BS_COLS) {                       // causal
      const int nc = min(BS_COLS, SX - c0);
      load_source(c0, nc, true, true);
      __syncthreads();
      if (walks)
        for (int c = 0; c < nc; ++c) {
          const double cur = c0 + c == 0 ? bs_causal_first(st) : bs_causal_step(tile[row][c], st.last, z);
          tile[row][c] = cur;
          st.before = st.last;
          st.last = cur;
        }
      __syncthreads();
      store_coeffs(c0, nc);
      __syncthreads();
    }
    for (int c0 = last_c0; c0 >= 0; c0 -= BS_COLS) {                 // anti-causal, over the c+ just written by this workgroup
      const int nc = min(BS_COLS, SX - c0);
      bs_chunk(nrows, nc, [&](int r, int c) { tile[r][c] = coeffs[base + (int64_t)r * SX + c0 + c]; });
      __syncthreads();
      if (walks)
        for (int c = nc - 1; c >= 0; --c) {
          const double cur = c0 + c == SX - 1 ? bs_anticausal_first(st.last, st.before, z) : bs_anticausal_step(st.last, tile[row][c], z);
          tile[row][c] = cur;
          st.last = cur;
        }
      __syncthreads();
      store_coeffs(c0, nc);
      __syncthreads();
    }
  }
  if (bad) atomicAdd(&s_bad, bad);
  vc_hist_merge(&s_bad, 1, nonfinite);
}

// ---- the y and z passes: in place, one thread per line, `stride` elements between the positions of a line (N >= 2) -----------------------
__global__ __launch_bounds__(VI_THREADS) void k_bs_line(double* coeffs, int64_t cols, int64_t lines, int64_t plane_stride, int64_t stride, int N,
                                                        double z) {
  VI_GRID_STRIDE(l, lines) {
    const int64_t plane = l / cols;
    double* p = coeffs + plane * plane_stride + (l - plane * cols);
    bs_line_state st = {0.0, 1.0, 0.0, 0.0};
    for (int i = 0; i < N; ++i) bs_sum_step(st, bs_times6(p[i * stride]), z);
    for (int i = N - 2; i >= 1; --i) bs_sum_step(st, bs_times6(p[i * stride]), z);
    st.last = bs_causal_first(st);
    p[0] = st.last;
    for (int i = 1; i < N; ++i) {
      const double cur = bs_causal_step(bs_times6(p[i * stride]), st.last, z);
      p[i * stride] = cur;
      st.before = st.last;
      st.last = cur;
    }
    st.last = bs_anticausal_first(st.last, st.before, z);
    p[(N - 1) * stride] = st.last;
    for (int i = N - 2; i >= 0; --i) {
      st.last = bs_anticausal_step(st.last, p[i * stride], z);
      p[i * stride] = st.last;
    }
  }
}

extern "C" int mud_volume_bspline_coeffs(const void* vol, int datatype, int SX, int SY, int SZ, float slope, float inter, double* coeffs,
                                         uint32_t* nonfinite, void* stream) {
  MUD_REQUIRE(vol != nullptr, "mud_volume_bspline_coeffs: null pointer (vol)");
  if (int e = vi_check_volume("mud_volume_bspline_coeffs", vol, datatype, SX, SY, SZ)) return e;
  MUD_REQUIRE(coeffs != nullptr, "mud_volume_bspline_coeffs: null pointer (coeffs)");
  MUD_REQUIRE(nonfinite != nullptr, "mud_volume_bspline_coeffs: null pointer (nonfinite)");
  MUD_REQUIRE(mud_aligned16(coeffs) && vi_aligned(nonfinite, 4), "mud_volume_bspline_coeffs: coeffs must be 16-byte, nonfinite 4-byte aligned");
  MUD_REQUIRE((const void*)coeffs != vol, "mud_volume_bspline_coeffs: coeffs must be a buffer of its own");
  hipStream_t s = (hipStream_t)stream;
  if (int e = vi_clear("mud_volume_bspline_coeffs", nonfinite, sizeof(uint32_t), s)) return e;
  const double z = std::sqrt(3.0) - 2.0;
  const int64_t XY = (int64_t)SX * SY, nlines = (int64_t)SY * SZ;
  VI_DISPATCH(datatype, hipLaunchKernelGGL(k_bs_x<T>, dim3((unsigned)mud_cdiv(nlines, BS_ROWS)), dim3(VI_THREADS), 0, s,
                                           vi_source_of(vol, datatype, slope, inter), SX, nlines, z, coeffs, nonfinite));
  MUD_CHECK_LAUNCH("mud_volume_bspline_coeffs (x)");
  if (SY > 1) {                                // a plane per z, the lines of a plane at adjacent x
    const int64_t lines = (int64_t)SX * SZ;
    hipLaunchKernelGGL(k_bs_line, dim3(vi_blocks(lines)), dim3(VI_THREADS), 0, s, coeffs, (int64_t)SX, lines, XY, (int64_t)SX, SY, z);
    MUD_CHECK_LAUNCH("mud_volume_bspline_coeffs (y)");
  }
  if (SZ > 1) {                                // one plane, the lines at adjacent x + SX y
    hipLaunchKernelGGL(k_bs_line, dim3(vi_blocks(XY)), dim3(VI_THREADS), 0, s, coeffs, XY, XY, (int64_t)0, XY, SZ, z);
    MUD_CHECK_LAUNCH("mud_volume_bspline_coeffs (z)");
  }
  return MUD_OK;
}

// ---- the interpolation -----------------------------------------------------------------------------------------------------------------
// p = m (i, j, k, 1), every product and sum rounded separately, left to right (tests/volume_regrid_ref.py: coordinates)
__device__ __forceinline__ void bs_coordinate(const vi_mat& M, double x, double y, double z, double p[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double px = M.m[4 * a] * x, py = M.m[4 * a + 1] * y, pz = M.m[4 * a + 2] * z;
    double s = px + py;
    s = s + pz;
    p[a] = s + M.m[4 * a + 3];
  }
}

// the four weights of mud_volume_bias_* (volume_bias.hip: vb_axis) at t in [0, 1)
__device__ __forceinline__ void bs_weights(double t, double b[4]) {
#pragma clang fp contract(off)
  const double omt = 1.0 - t, t2 = t * t;
  const double t3 = t2 * t;
  b[0] = ((omt * omt) * omt) / 6.0;
  b[1] = ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0;
  b[2] = (((3.0 * t2 - 3.0 * t3) + 3.0 * t) + 1.0) / 6.0;
  b[3] = t3 / 6.0;
}

// index i in [-1, S + 1] of an axis of S under mirror boundaries.  The last step serves S = 2 alone (3 -> -1 -> 1, reached only at
// p = 1 exactly, with weight 0)
__device__ __forceinline__ int bs_mirror(int i, int S) {
  if (S == 1) return 0;
  if (i < 0) i = -i;
  if (i > S - 1) i = 2 * (S - 1) - i;
  return i < 0 ? -i : i;
}

// the background guard: is any in-volume trilinear neighbour of non-zero weight a voxel whose value is not 0?
template <typename T>
__device__ __forceinline__ bool bs_tissue(const vi_source& src, int SX, int SY, int SZ, const int f[3], const double t[3]) {
#pragma clang fp contract(off)
  const double wx[2] = {1.0 - t[0], t[0]}, wy[2] = {1.0 - t[1], t[1]}, wz[2] = {1.0 - t[2], t[2]};
  bool tissue = false;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
    const int xx = f[0] + dx, yy = f[1] + dy, zz = f[2] + dz;
    const double w = (wx[dx] * wy[dy]) * wz[dz];
    if (w != 0.0 && xx < SX && yy < SY && zz < SZ && vi_at<T>(src, ((int64_t)zz * SY + yy) * SX + xx) != 0.0f) tissue = true;
  }
  return tissue;
}

template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_bs_regrid(const double* __restrict__ coeffs, vi_source src, int SX, int SY, int SZ, vi_mat M,
                                                          double lo, double hi, int X, int Y, int64_t n, float* __restrict__ out) {
#pragma clang fp contract(off)
  VI_GRID_STRIDE(i, n) {
    int x, y, z;
    vi_xyz(i, X, Y, x, y, z);
    double p[3];
    bs_coordinate(M, (double)x, (double)y, (double)z, p);
    float r = 0.0f;
    if (p[0] >= 0.0 && p[0] <= (double)(SX - 1) && p[1] >= 0.0 && p[1] <= (double)(SY - 1) && p[2] >= 0.0 && p[2] <= (double)(SZ - 1)) {
      const double fl[3] = {floor(p[0]), floor(p[1]), floor(p[2])};
      const double t[3] = {p[0] - fl[0], p[1] - fl[1], p[2] - fl[2]};
      const int f[3] = {(int)fl[0], (int)fl[1], (int)fl[2]};
      if (bs_tissue<T>(src, SX, SY, SZ, f, t)) {
        double bx[4], by[4], bz[4];
        bs_weights(t[0], bx);
        bs_weights(t[1], by);
        bs_weights(t[2], bz);
        int ix[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) ix[d] = bs_mirror(f[0] - 1 + d, SX);
        double acc = 0.0;
#pragma unroll
        for (int dz = 0; dz < 4; ++dz) {
          const int64_t pz = (int64_t)bs_mirror(f[2] - 1 + dz, SZ) * SY;
#pragma unroll
          for (int dy = 0; dy < 4; ++dy) {
            const double* row = coeffs + (pz + bs_mirror(f[1] - 1 + dy, SY)) * SX;
#pragma unroll
            for (int dx = 0; dx < 4; ++dx) {
              const double w = (bx[dx] * by[dy]) * bz[dz];
              const double term = w * row[ix[dx]];
              acc = acc + term;
            }
          }
        }
        acc = acc < lo ? lo : acc;
        acc = acc > hi ? hi : acc;
        r = (float)acc;
      }
    }
    out[i] = r;
  }
}

extern "C" int mud_volume_regrid_cubic(const double* coeffs, int SX, int SY, int SZ, const void* src, int datatype, float slope, float inter,
                                       const double* m, double lo, double hi, int X, int Y, int Z, float* out, void* stream) {
  MUD_REQUIRE(src != nullptr, "mud_volume_regrid_cubic: null pointer (src)");
  if (int e = vi_check_volume("mud_volume_regrid_cubic", src, datatype, SX, SY, SZ)) return e;
  if (int e = vi_check_size("mud_volume_regrid_cubic", "output", X, Y, Z)) return e;
  MUD_REQUIRE(coeffs != nullptr, "mud_volume_regrid_cubic: null pointer (coeffs)");
  MUD_REQUIRE(m != nullptr, "mud_volume_regrid_cubic: null pointer (m)");
  MUD_REQUIRE(out != nullptr, "mud_volume_regrid_cubic: null pointer (out)");
  MUD_REQUIRE(vi_aligned(coeffs, 8), "mud_volume_regrid_cubic: coeffs must be 8-byte aligned");
  MUD_REQUIRE(lo - lo == 0.0 && hi - hi == 0.0 && lo <= 0.0 && hi >= 0.0, "mud_volume_regrid_cubic: lo / hi must be finite with lo <= 0 <= hi (%g, %g)",
              lo, hi);
  vi_mat M;
  for (int i = 0; i < 12; ++i) {
    MUD_REQUIRE(m[i] - m[i] == 0.0, "mud_volume_regrid_cubic: m[%d] = %g is not finite", i, m[i]);
    M.m[i] = m[i];
  }
  const int64_t n = (int64_t)X * Y * Z;
  VI_DISPATCH(datatype, hipLaunchKernelGGL(k_bs_regrid<T>, dim3(vi_blocks(n)), dim3(VI_THREADS), 0, (hipStream_t)stream, coeffs,
                                           vi_source_of(src, datatype, slope, inter), SX, SY, SZ, M, lo, hi, X, Y, n, out));
  MUD_CHECK_LAUNCH("mud_volume_regrid_cubic");
  return MUD_OK;
}
