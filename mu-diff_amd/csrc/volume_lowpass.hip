// The low-pass in front of a resampling that downsamples (--antialias / --conform; include/mudiff_hip.h: mud_volume_lowpass;
// mudiff_hip.volume_conform): a separable Gaussian whose weights the host computed in fp64, one pass per axis
// in x, y, z order, a pass whose weights are absent skipped.  One pass along axis a:
//
//     out[i] = (sum_t w[t] v[i + t]) / (sum_t w[t]),  both sums over the t in [-R, R] with 0 <= i + t < S_a, t ascending
//
// truncation with renormalisation: nothing is invented outside the field of view and the edge does not darken.  Products and sums
// are fp64 (an fma per tap), the quotient is rounded to fp32 once.  v is the value of the stored voxel (vi_value) on the first pass
// that runs and the fp32 of the pass before on the later ones; a non-finite v is read as 0, and counted on the first pass.
//
// Every global access runs along x, whatever the axis:
//   x pass    (k_vl_rows)  a workgroup stages VL_SEG voxels of one row plus R on either side in LDS; a thread owns one output.
//   y, z pass (k_vl_cols)  a workgroup stages an x-run of VL_RUN voxels times VL_T + 2 R positions along the filtered axis; the 64 lanes
//             of a wave lie along x, in global memory (one run of 64 elements per row of the tile) and in LDS (64 consecutive
//             dwords: 64 different banks), and each wave walks the filtered axis.  No lane walks a strided column.
// Sub-dword datatypes are read four or two voxels to a dword (vo_load: rows start where they start, so the dword is of unknown
// alignment); a dword that would cross the end of the row falls back to single elements.  The tile holds the fp32 values, so the
// taps read LDS only.  The weights travel in the kernel arguments (33 doubles) and are indexed by the loop counter alone, which is
// uniform: they stay in scalar registers.
#include "volume_common.h"

#define VL_MAX_R 16
#define VL_SEG VI_THREADS                      // outputs of one piece of work of the x pass
#define VL_RUN 64                              // the x-run of the y / z passes: one wave
#define VL_T 32                                // outputs along the filtered axis per piece of work of the y / z passes
#define VL_WAVES (VI_THREADS / VL_RUN)
#define VL_MAX_BLOCKS 8192

struct vl_pass {
  double w[2 * VL_MAX_R + 1];                  // w[t + R], t = -R..R
  int R;
  int X, Y, Z;
  int SA, SO;                                  // y / z pass: the extents along the filtered axis and along the third one ...
  int64_t stride_a, stride_o;                  // ... and their strides in voxels (x: 1)
};

// the value the filter sees: a non-finite one is 0; *bad counts those of the voxels this piece of work owns
template <typename T>
__device__ __forceinline__ float vl_value(const vi_source& s, T raw, bool own, uint32_t& bad) {
  float v = vi_value<T>(raw, s.scaled, s.slope, s.inter);
  if (!vc_finite(v)) {
    bad += own ? 1u : 0u;
    v = 0.0f;
  }
  return v;
}

// n voxels of one row, from p on, to tile[0..n): a dword of V voxels per step where it fits, single voxels at the end.  `own0`,
// `own1`: the positions [own0, own1) of those n belong to this piece of work (the rest is halo)
template <typename T>
__device__ __forceinline__ void vl_stage(const vi_source& s, const T* p, int e, int n, float* tile, int own0, int own1, uint32_t& bad) {
  constexpr int V = 4 / (int)sizeof(T);
  if (V > 1 && e + V <= n) {
    const uint32_t w = vo_load<uint32_t>(p + e);
#pragma unroll
    for (int k = 0; k < V; ++k) tile[e + k] = vl_value<T>(s, vo_element<T, uint32_t>(w, k), e + k >= own0 && e + k < own1, bad);
  } else {
    for (int k = 0; k < V && e + k < n; ++k) tile[e + k] = vl_value<T>(s, p[e + k], e + k >= own0 && e + k < own1, bad);
  }
}

// the taps of one output at position i of an axis of extent S; `at`: the tile entry of position i, `step`: entries per position
__device__ __forceinline__ float vl_taps(const vl_pass& g, const float* at, int step, int i, int S) {
  double acc = 0.0, den = 0.0;
  for (int t = -g.R; t <= g.R; ++t) {
    const double w = g.w[t + g.R];
    if (i + t >= 0 && i + t < S) {
      acc = fma(w, (double)at[t * step], acc);
      den += w;
    }
  }
  return (float)(acc / den);
}

template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_vl_rows(vi_source src, float* __restrict__ dst, vl_pass g, uint32_t* __restrict__ nonfinite) {
  constexpr int V = 4 / (int)sizeof(T);
  __shared__ float tile[VL_SEG + 2 * VL_MAX_R];
  __shared__ uint32_t s_bad;
  vc_hist_clear(&s_bad, 1);
  uint32_t bad = 0;
  const int segs = (g.X + VL_SEG - 1) / VL_SEG;
  const int64_t total = (int64_t)segs * g.Y * g.Z;
  for (int64_t work = blockIdx.x; work < total; work += gridDim.x) {
    const int64_t row = work / segs;
    const int x0 = (int)(work - row * segs) * VL_SEG;
    const int lo = max(x0 - g.R, 0), hi = min(x0 + VL_SEG + g.R, g.X);      // what is staged: tile[0] is position lo
    const T* p = (const T*)src.vol + row * g.X + lo;
    for (int q = threadIdx.x; q * V < hi - lo; q += VI_THREADS)
      vl_stage<T>(src, p, q * V, hi - lo, tile, x0 - lo, x0 - lo + VL_SEG, bad);
    __syncthreads();
    const int x = x0 + (int)threadIdx.x;
    if (x < g.X) dst[row * g.X + x] = vl_taps(g, tile + (x - lo), 1, x, g.X);
    __syncthreads();                           // the tile is free for the next piece of work
  }
  if (nonfinite) {                             // (uniform over the launch)
    if (bad) atomicAdd(&s_bad, bad);
    vc_hist_merge(&s_bad, 1, nonfinite);
  }
}

template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_vl_cols(vi_source src, float* __restrict__ dst, vl_pass g, uint32_t* __restrict__ nonfinite) {
  constexpr int V = 4 / (int)sizeof(T), WPR = VL_RUN / V;                    // dwords of V voxels per row of the tile
  __shared__ float tile[(VL_T + 2 * VL_MAX_R) * VL_RUN];
  __shared__ uint32_t s_bad;
  vc_hist_clear(&s_bad, 1);
  uint32_t bad = 0;
  const int runs = (g.X + VL_RUN - 1) / VL_RUN, tiles = (g.SA + VL_T - 1) / VL_T;
  const int64_t per_o = (int64_t)runs * tiles, total = per_o * g.SO;
  const int lane = threadIdx.x % VL_RUN, wave = threadIdx.x / VL_RUN;
  for (int64_t work = blockIdx.x; work < total; work += gridDim.x) {
    const int64_t o = work / per_o;
    const int rem = (int)(work - o * per_o);
    const int x0 = (rem % runs) * VL_RUN, a0 = (rem / runs) * VL_T;
    const int lo = max(a0 - g.R, 0), hi = min(a0 + VL_T + g.R, g.SA);       // the positions along the axis that are staged
    const int n = min(VL_RUN, g.X - x0);                                    // the voxels of this x-run
    const int64_t base = o * g.stride_o + x0;
    for (int q = threadIdx.x; q < (hi - lo) * WPR; q += VI_THREADS) {
      const int r = q / WPR, e = (q % WPR) * V;
      if (e >= n) continue;
      const bool own = lo + r >= a0 && lo + r < a0 + VL_T;
      vl_stage<T>(src, (const T*)src.vol + base + (lo + r) * g.stride_a, e, n, tile + r * VL_RUN, own ? 0 : n, n, bad);
    }
    __syncthreads();
    if (lane < n) {
      for (int j = wave; j < VL_T && a0 + j < g.SA; j += VL_WAVES) {
        const int a = a0 + j;
        dst[base + a * g.stride_a + lane] = vl_taps(g, tile + (a - lo) * VL_RUN + lane, VL_RUN, a, g.SA);
      }
    }
    __syncthreads();                           // the tile is free for the next piece of work
  }
  if (nonfinite) {
    if (bad) atomicAdd(&s_bad, bad);
    vc_hist_merge(&s_bad, 1, nonfinite);
  }
}

template <typename T>
static void vl_launch(int axis, const vi_source& src, float* dst, vl_pass g, uint32_t* nonfinite, hipStream_t s) {
  if (axis == 0) {
    const int64_t total = mud_cdiv(g.X, VL_SEG) * g.Y * g.Z;
    hipLaunchKernelGGL(k_vl_rows<T>, dim3(vi_blocks(total, 1, VL_MAX_BLOCKS)), dim3(VI_THREADS), 0, s, src, dst, g, nonfinite);
    return;
  }
  g.SA = axis == 1 ? g.Y : g.Z, g.SO = axis == 1 ? g.Z : g.Y;
  g.stride_a = axis == 1 ? g.X : (int64_t)g.X * g.Y, g.stride_o = axis == 1 ? (int64_t)g.X * g.Y : g.X;
  const int64_t total = mud_cdiv(g.X, VL_RUN) * mud_cdiv(g.SA, VL_T) * g.SO;
  hipLaunchKernelGGL(k_vl_cols<T>, dim3(vi_blocks(total, 1, VL_MAX_BLOCKS)), dim3(VI_THREADS), 0, s, src, dst, g, nonfinite);
}

static bool vl_disjoint(const void* a, uintptr_t a_bytes, const void* b, uintptr_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 + a_bytes <= b0 || b0 + b_bytes <= a0;
}

extern "C" int mud_volume_lowpass(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, const double* wx, int rx,
                                  const double* wy, int ry, const double* wz, int rz, float* out, float* scratch, uint32_t* nonfinite,
                                  void* stream) {
  const char* who = "mud_volume_lowpass";
  const double* W[3] = {wx, wy, wz};
  const int R[3] = {rx, ry, rz};
  int passes = 0;
  for (int a = 0; a < 3; ++a) {
    if (W[a] == nullptr) continue;             // this axis is not filtered
    ++passes;
    MUD_REQUIRE(R[a] >= 0 && R[a] <= VL_MAX_R, "%s: axis %d: the radius must be in [0, %d], got %d", who, a, VL_MAX_R, R[a]);
    for (int t = 0; t <= 2 * R[a]; ++t)
      MUD_REQUIRE(W[a][t] - W[a][t] == 0.0 && W[a][t] >= 0.0, "%s: axis %d: weight %d is %g (finite and not negative)", who, a, t - R[a], W[a][t]);
    MUD_REQUIRE(W[a][R[a]] > 0.0, "%s: axis %d: the centre weight must be positive", who, a);
  }
  if (int e = vi_check_volume(who, vol, datatype, X, Y, Z)) return e;
  if (passes == 0) return MUD_OK;              // nothing to filter: nothing is launched and nothing is written
  MUD_REQUIRE(out != nullptr && nonfinite != nullptr && (passes < 2 || scratch != nullptr), "%s: null pointer", who);
  MUD_REQUIRE(mud_aligned16(out) && (passes < 2 || mud_aligned16(scratch)), "%s: the output and the scratch volume must be 16-byte aligned", who);
  MUD_REQUIRE(vi_aligned(nonfinite, 4), "%s: the counter must be 4-byte aligned", who);
  const uintptr_t n = (uintptr_t)X * Y * Z, src_bytes = n * vi_esize(datatype), f_bytes = n * 4;
  MUD_REQUIRE(vl_disjoint(out, f_bytes, vol, src_bytes), "%s: the output overlaps the source", who);
  MUD_REQUIRE(vl_disjoint(nonfinite, 4, out, f_bytes), "%s: the counter lies inside the output", who);
  if (passes >= 2) {
    MUD_REQUIRE(vl_disjoint(out, f_bytes, scratch, f_bytes), "%s: the output overlaps the scratch volume", who);
    MUD_REQUIRE(vl_disjoint(scratch, f_bytes, vol, src_bytes), "%s: the scratch volume overlaps the source", who);
    MUD_REQUIRE(vl_disjoint(nonfinite, 4, scratch, f_bytes), "%s: the counter lies inside the scratch volume", who);
  }
  hipStream_t s = (hipStream_t)stream;
  if (int e = vi_clear(who, nonfinite, 4, s)) return e;
  // the last pass writes `out`, the one before it `scratch`, the one before that `out` again
  vi_source src = vi_source_of(vol, datatype, slope, inter);
  int left = passes;
  for (int a = 0; a < 3; ++a) {
    if (W[a] == nullptr) continue;
    vl_pass g = {};
    for (int t = 0; t <= 2 * R[a]; ++t) g.w[t] = W[a][t];
    g.R = R[a], g.X = X, g.Y = Y, g.Z = Z;
    float* dst = (left & 1) ? out : scratch;
    uint32_t* count = left == passes ? nonfinite : nullptr;      // the first pass reads the stored voxels and counts
    VI_DISPATCH(src.datatype, vl_launch<T>(a, src, dst, g, count, s));
    MUD_CHECK_LAUNCH(who);
    src = vi_source_of(dst, MUD_NIFTI_F4, 1.0f, 0.0f);
    --left;
  }
  return MUD_OK;
}
