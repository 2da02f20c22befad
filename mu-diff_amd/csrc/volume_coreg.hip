// Rigid co-registration of the volume pipeline's inputs (--coregister; include/mudiff_hip.h: mud_volume_joint_hist;
// mudiff_hip.volume_coreg).
//
// The search for the six rigid parameters runs on the host; what it evaluates, many hundred times per volume, is the joint histogram of
// the fixed volume and the moving volume seen through a candidate matrix.  That histogram is this kernel: one thread per sample point
// of the fixed grid (every stride-th voxel per axis), the moving value by volume_common.h's trilinear rule - the voxel mud_volume_regrid
// would write there - both values binned in fp64 and counted in volume_common.h's LDS histogram.  Integer counts: the result does not
// depend on the order of arrival.
// Only the overlap counts: a sample whose moving coordinate leaves [0, S - 1] on any axis, or whose values are not both finite, is
// not counted, so that no zero padding enters the measure.
#include "volume_common.h"

#define VC_MAX_BINS 64
#define VC_MAX_BLOCKS 1024                     // 4 workgroups per CU: each merges up to bins^2 counts, so fewer, longer-lived groups

struct vc_side {                               // one volume: how to read it, how to bin it
  vi_source src;
  double lo, scale;
};

template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_vc_joint_hist(vc_side fix, int X, int Y, vc_side mov, int SX, int SY, int SZ, vi_mat M, int stride,
                                                              int nx, int ny, int64_t n, int bins, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[VC_MAX_BINS * VC_MAX_BINS];
  const int nb = bins * bins;                  // <= VC_MAX_BINS^2 (the entry point checks it)
  vc_hist_clear(h, nb);
  VI_GRID_STRIDE(i, n) {
    int xi, yj, zk;
    vi_xyz(i, nx, ny, xi, yj, zk);
    xi *= stride, yj *= stride, zk *= stride;
    double p[3];
    vi_coordinate(M, (double)xi, (double)yj, (double)zk, p);
    // the overlap: 0 <= p <= S - 1 on every axis (a NaN fails); inside it every neighbour of non-zero weight is a stored voxel
    if (!(p[0] >= 0.0 && p[0] <= (double)(SX - 1) && p[1] >= 0.0 && p[1] <= (double)(SY - 1) && p[2] >= 0.0 && p[2] <= (double)(SZ - 1))) continue;
    const float fv = vc_stored_value(fix.src, ((int64_t)zk * Y + yj) * X + xi);
    const float mv = vi_trilinear<T>(mov.src, SX, SY, SZ, p);
    if (!vc_finite(fv) || !vc_finite(mv)) continue;
    atomicAdd(&h[vc_bin(fv, fix.lo, fix.scale, bins) * bins + vc_bin(mv, mov.lo, mov.scale, bins)], 1u);
  }
  vc_hist_merge(h, nb, hist);
}

extern "C" int mud_volume_joint_hist(const void* fix, int fix_dt, int X, int Y, int Z, float fix_slope, float fix_inter, const void* mov,
                                     int mov_dt, int SX, int SY, int SZ, float mov_slope, float mov_inter, const double* m, int stride,
                                     double fix_lo, double fix_scale, double mov_lo, double mov_scale, int bins, uint32_t* hist, void* stream) {
  if (int e = vi_check_volume("mud_volume_joint_hist (fixed)", fix, fix_dt, X, Y, Z)) return e;
  if (int e = vi_check_volume("mud_volume_joint_hist (moving)", mov, mov_dt, SX, SY, SZ)) return e;
  MUD_REQUIRE(m != nullptr && hist != nullptr, "mud_volume_joint_hist: null pointer");
  MUD_REQUIRE(vi_aligned(hist, 4), "mud_volume_joint_hist: hist must be 4-byte aligned");
  MUD_REQUIRE(stride > 0, "mud_volume_joint_hist: stride %d is not positive", stride);
  if (int e = vi_check_bins("mud_volume_joint_hist (fixed)", fix_lo, fix_scale, bins, 2, VC_MAX_BINS)) return e;
  if (int e = vi_check_bins("mud_volume_joint_hist (moving)", mov_lo, mov_scale, bins, 2, VC_MAX_BINS)) return e;
  vi_mat M;
  for (int i = 0; i < 12; ++i) {
    MUD_REQUIRE(m[i] - m[i] == 0.0, "mud_volume_joint_hist: m[%d] = %g is not finite", i, m[i]);
    M.m[i] = m[i];
  }
  hipStream_t s = (hipStream_t)stream;
  const int nx = (int)mud_cdiv(X, stride), ny = (int)mud_cdiv(Y, stride), nz = (int)mud_cdiv(Z, stride);
  const int64_t n = (int64_t)nx * ny * nz;
  if (int e = vi_clear("mud_volume_joint_hist", hist, sizeof(uint32_t) * bins * bins, s)) return e;
  const vc_side f = {vi_source_of(fix, fix_dt, fix_slope, fix_inter), fix_lo, fix_scale};
  const vc_side v = {vi_source_of(mov, mov_dt, mov_slope, mov_inter), mov_lo, mov_scale};
  VI_DISPATCH(mov_dt, hipLaunchKernelGGL(k_vc_joint_hist<T>, dim3(vi_blocks(n, VI_THREADS, VC_MAX_BLOCKS)), dim3(VI_THREADS), 0, s, f, X, Y, v, SX, SY,
                                         SZ, M, stride, nx, ny, n, bins, hist));
  MUD_CHECK_LAUNCH("mud_volume_joint_hist");
  return MUD_OK;
}
