// Rigid co-registration of the volume pipeline's inputs (--coregister; include/mudiff_hip.h: mud_volume_joint_hist;
// mudiff_hip.volume_coreg).
//
// The search for the six rigid parameters runs on the host; what it evaluates, many hundred times per volume, is the joint histogram of
// the fixed volume and the moving volume seen through a candidate matrix.  That histogram is this kernel: one thread per sample point
// of the fixed grid (every stride-th voxel per axis), the moving value by volume_common.h's trilinear rule - the voxel mud_volume_regrid
// would write there - both values binned in fp64, counted in a per-workgroup LDS histogram with integer atomics and merged into the
// global one with one integer atomic per non-empty bin.  Integer counts: the result does not depend on the order of arrival.
// Only the overlap counts: a sample whose moving coordinate leaves [0, S - 1] on any axis, or whose values are not both finite, is
// not counted, so that no zero padding enters the measure.
#include "volume_common.h"

#define VC_MAX_BINS 64
#define VC_MAX_BLOCKS 1024                     // 4 workgroups per CU: each merges up to bins^2 counts, so fewer, longer-lived groups

struct vc_side {                               // one volume: stored voxels, how to read them, how to bin them
  const void* vol;
  int datatype, scaled;
  double slope, inter, lo, scale;
};

template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_vc_joint_hist(vc_side fix, int X, int Y, vc_side mov, int SX, int SY, int SZ, vi_mat M, int stride,
                                                              int nx, int ny, int64_t n, int bins, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[VC_MAX_BINS * VC_MAX_BINS];
  const int nb = bins * bins;                  // <= VC_MAX_BINS^2 (the entry point checks it)
  for (int i = threadIdx.x; i < nb; i += VI_THREADS) h[i] = 0;
  __syncthreads();
  const T* __restrict__ src = (const T*)mov.vol;
  for (int64_t i = (int64_t)blockIdx.x * VI_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * VI_THREADS) {
    const uint32_t l = (uint32_t)i;                          // n <= X*Y*Z < 2^31: 32-bit divisions
    const uint32_t row = l / (uint32_t)nx;
    const int xi = (int)(l - row * (uint32_t)nx) * stride, yj = (int)(row % (uint32_t)ny) * stride, zk = (int)(row / (uint32_t)ny) * stride;
    double p[3];
    vi_coordinate(M, (double)xi, (double)yj, (double)zk, p);
    // the overlap: 0 <= p <= S - 1 on every axis (a NaN fails); inside it every neighbour of non-zero weight is a stored voxel
    if (!(p[0] >= 0.0 && p[0] <= (double)(SX - 1) && p[1] >= 0.0 && p[1] <= (double)(SY - 1) && p[2] >= 0.0 && p[2] <= (double)(SZ - 1))) continue;
    const float fv = vc_stored_value(fix.vol, fix.datatype, ((int64_t)zk * Y + yj) * X + xi, fix.scaled, fix.slope, fix.inter);
    const float mv = vi_trilinear<T>(src, SX, SY, SZ, mov.scaled, mov.slope, mov.inter, p);
    if (!vc_finite(fv) || !vc_finite(mv)) continue;
    atomicAdd(&h[vc_bin(fv, fix.lo, fix.scale, bins) * bins + vc_bin(mv, mov.lo, mov.scale, bins)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += VI_THREADS) {
    const uint32_t c = h[i];
    if (c) atomicAdd(&hist[i], c);
  }
}

extern "C" int mud_volume_joint_hist(const void* fix, int fix_dt, int X, int Y, int Z, float fix_slope, float fix_inter, const void* mov,
                                     int mov_dt, int SX, int SY, int SZ, float mov_slope, float mov_inter, const double* m, int stride,
                                     double fix_lo, double fix_scale, double mov_lo, double mov_scale, int bins, uint32_t* hist, void* stream) {
  if (int e = vi_check_volume("mud_volume_joint_hist (fixed)", fix, fix_dt, X, Y, Z)) return e;
  if (int e = vi_check_volume("mud_volume_joint_hist (moving)", mov, mov_dt, SX, SY, SZ)) return e;
  MUD_REQUIRE(m != nullptr && hist != nullptr, "mud_volume_joint_hist: null pointer");
  MUD_REQUIRE((((uintptr_t)hist) & 3u) == 0, "mud_volume_joint_hist: hist must be 4-byte aligned");
  MUD_REQUIRE(stride > 0, "mud_volume_joint_hist: stride %d is not positive", stride);
  MUD_REQUIRE(bins >= 2 && bins <= VC_MAX_BINS, "mud_volume_joint_hist: 2 to %d bins, got %d", VC_MAX_BINS, bins);
  vi_mat M;
  for (int i = 0; i < 12; ++i) {
    MUD_REQUIRE(m[i] - m[i] == 0.0, "mud_volume_joint_hist: m[%d] = %g is not finite", i, m[i]);
    M.m[i] = m[i];
  }
  MUD_REQUIRE(fix_lo - fix_lo == 0.0 && fix_scale - fix_scale == 0.0 && mov_lo - mov_lo == 0.0 && mov_scale - mov_scale == 0.0,
              "mud_volume_joint_hist: lo / scale must be finite (%g, %g, %g, %g)", fix_lo, fix_scale, mov_lo, mov_scale);
  hipStream_t s = (hipStream_t)stream;
  const int nx = (int)mud_cdiv(X, stride), ny = (int)mud_cdiv(Y, stride), nz = (int)mud_cdiv(Z, stride);
  const int64_t n = (int64_t)nx * ny * nz;
  int64_t blocks = mud_cdiv(n, VI_THREADS);
  blocks = blocks > VC_MAX_BLOCKS ? VC_MAX_BLOCKS : blocks;
  if (hipMemsetAsync(hist, 0, sizeof(uint32_t) * bins * bins, s) != hipSuccess) {
    mud_set_error("mud_volume_joint_hist: clearing the histogram failed");
    return MUD_ERR_LAUNCH;
  }
  const vc_side f = {fix, fix_dt, vi_scaled(fix_slope, fix_inter), (double)fix_slope, (double)fix_inter, fix_lo, fix_scale};
  const vc_side v = {mov, mov_dt, vi_scaled(mov_slope, mov_inter), (double)mov_slope, (double)mov_inter, mov_lo, mov_scale};
  VI_DISPATCH(mov_dt, hipLaunchKernelGGL(k_vc_joint_hist<T>, dim3((unsigned)blocks), dim3(VI_THREADS), 0, s, f, X, Y, v, SX, SY, SZ, M, stride, nx,
                                         ny, n, bins, hist));
  MUD_CHECK_LAUNCH("mud_volume_joint_hist");
  return MUD_OK;
}
