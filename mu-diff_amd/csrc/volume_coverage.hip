// Interval coverage of an ensemble's quantile maps against a ground truth (include/mudiff_hip.h: mud_volume_interval_coverage;
// mudiff_hip.volume_coverage): per plane of a [Z, X, Y] slab and per region (bit k of a uint8 per voxel, as
// volume_metrics.hip reads it) how many voxels of the ground truth lie below, inside and above the interval [lo, hi], and the fp64 sums of
// the interval's width over all of them and over the covered ones.  A std / error correlation says that the spread is larger where the
// error is; whether a nominal 90 % interval holds the truth 90 % of the time is this count.
//
// The reduction is the one of volume_metrics.hip and volume_through_plane.hip: partials per (plane, workgroup, region) go to a workspace
// and a second kernel adds a plane's partials in workgroup order.  The counts travel as fp64 (exact below 2^53; a volume has fewer than
// 2^31 voxels) and leave as int64.  No atomics: the same bits on every run.
#include "volume_common.h"

#define VC_THREADS 256
#define VC_WAVES (VC_THREADS / 64)
#define VC_PARTS MUD_VC_PARTS
#define VC_NQ (MUD_VC_NC + MUD_VC_NS)          // a partial's slots: the MUD_VC_NC counts, then the MUD_VC_NS sums
#define VC_MAX_REG MUD_VM_MAX_REGIONS

// workgroup (plane zi, part p): the voxels p * VC_THREADS + t, + VC_PARTS * VC_THREADS, ... of plane z0 + zi.  Every thread reaches the barrier.
__global__ __launch_bounds__(VC_THREADS) void k_volume_coverage(const float* __restrict__ lo, const float* __restrict__ hi, const float* __restrict__ gt,
                                                                const uint8_t* __restrict__ region, int64_t plane, int z0, int nreg,
                                                                double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[VC_WAVES][VC_MAX_REG][VC_NQ];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int p = blockIdx.x % VC_PARTS, zi = blockIdx.x / VC_PARTS;
  const int64_t base = (int64_t)(z0 + zi) * plane;
  double acc[VC_MAX_REG][VC_NQ];
#pragma unroll
  for (int k = 0; k < VC_MAX_REG; ++k)
#pragma unroll
    for (int q = 0; q < VC_NQ; ++q) acc[k][q] = 0.0;
  for (int64_t i = (int64_t)p * VC_THREADS + t; i < plane; i += (int64_t)VC_PARTS * VC_THREADS) {
    const float l = lo[base + i], h = hi[base + i], g = gt[base + i];
    const unsigned m = region ? region[base + i] : 0xffu;
    const bool nan = l != l || h != h || g != g;
    const bool below = !nan && g < l, above = !nan && g > h, inside = !nan && !below && !above;
    const double w = nan ? 0.0 : (double)h - (double)l;
#pragma unroll
    for (int k = 0; k < VC_MAX_REG; ++k) {
      if (k < nreg && ((m >> k) & 1u)) {
        acc[k][MUD_VC_N] += nan ? 0.0 : 1.0;
        acc[k][MUD_VC_BELOW] += below ? 1.0 : 0.0;
        acc[k][MUD_VC_ABOVE] += above ? 1.0 : 0.0;
        acc[k][MUD_VC_INSIDE] += inside ? 1.0 : 0.0;
        acc[k][MUD_VC_NONFINITE] += nan ? 1.0 : 0.0;
        acc[k][MUD_VC_NC + MUD_VC_WIDTH] += w;
        acc[k][MUD_VC_NC + MUD_VC_WIDTH_INSIDE] += inside ? w : 0.0;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < VC_MAX_REG; ++k) {
    if (k < nreg) {                                                     // uniform over the launch
#pragma unroll
      for (int q = 0; q < VC_NQ; ++q) {
        const double s = mud_wave_sum(acc[k][q]);
        if (lane == 0) red[wave][k][q] = s;
      }
    }
  }
  __syncthreads();
  if (t < nreg * VC_NQ) {
    const int k = t / VC_NQ, q = t - k * VC_NQ;
    double s = 0.0;
#pragma unroll
    for (int wv = 0; wv < VC_WAVES; ++wv) s += red[wv][k][q];
    part[(((int64_t)zi * VC_PARTS + p) * nreg + k) * VC_NQ + q] = s;
  }
}

// one lane per (plane, region, slot): the plane's partials in workgroup order; a count leaves as int64
__global__ __launch_bounds__(VC_THREADS) void k_volume_coverage_final(const double* __restrict__ part, int64_t n, int nreg,
                                                                      int64_t* __restrict__ counts, double* __restrict__ sums) {
  const int64_t i = (int64_t)blockIdx.x * VC_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t pr = i / VC_NQ, q = i - pr * VC_NQ;                      // pr = plane * nreg + region
  const int64_t zi = pr / nreg, k = pr - zi * nreg;
  double s = 0.0;
  for (int j = 0; j < VC_PARTS; ++j) s += part[((zi * VC_PARTS + j) * nreg + k) * VC_NQ + q];
  if (q < MUD_VC_NC)
    counts[pr * MUD_VC_NC + q] = (int64_t)s;
  else
    sums[pr * MUD_VC_NS + (q - MUD_VC_NC)] = s;
}

extern "C" int mud_volume_interval_coverage(const float* lo, const float* hi, const float* gt, const uint8_t* region, int Z, int X, int Y,
                                            int nreg, int z0, int z1, int64_t* counts, double* sums, void* ws, int64_t ws_bytes, void* stream) {
  if (int e = vi_check_size("mud_volume_interval_coverage", "volume", X, Y, Z)) return e;
  MUD_REQUIRE(nreg >= 1 && nreg <= VC_MAX_REG, "mud_volume_interval_coverage: nreg must be in [1, %d] (got %d)", VC_MAX_REG, nreg);
  MUD_REQUIRE(z0 >= 0 && z0 <= z1 && z1 < Z, "mud_volume_interval_coverage: planes %d..%d are not a range of the %d planes", z0, z1, Z);
  MUD_REQUIRE(lo && hi && gt && counts && sums && ws, "mud_volume_interval_coverage: null pointer");
  const int64_t planes = (int64_t)z1 - z0 + 1, need = planes * VC_PARTS * nreg * VC_NQ * 8;
  MUD_REQUIRE(planes * VC_PARTS <= 0x7fffffff, "mud_volume_interval_coverage: too many planes (%lld)", (long long)planes);
  MUD_REQUIRE(ws_bytes >= need, "mud_volume_interval_coverage: ws holds %lld bytes, needs %lld", (long long)ws_bytes, (long long)need);
  MUD_REQUIRE(vi_aligned(ws, 8) && vi_aligned(sums, 8) && vi_aligned(counts, 8) && vi_aligned(lo, 4) && vi_aligned(hi, 4) && vi_aligned(gt, 4),
              "mud_volume_interval_coverage: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_volume_coverage, dim3((unsigned)(planes * VC_PARTS)), dim3(VC_THREADS), 0, st, lo, hi, gt, region, (int64_t)X * Y, z0, nreg,
                     (double*)ws);
  hipLaunchKernelGGL(k_volume_coverage_final, dim3((unsigned)mud_cdiv(planes * nreg * VC_NQ, VC_THREADS)), dim3(VC_THREADS), 0, st,
                     (const double*)ws, planes * nreg * VC_NQ, nreg, counts, sums);
  MUD_CHECK_LAUNCH("mud_volume_interval_coverage");
  return MUD_OK;
}
