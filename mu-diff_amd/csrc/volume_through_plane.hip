// Through-plane roughness of a volume (include/mudiff_hip.h: mud_volume_through_plane; mudiff_hip.volume_through_plane, DESIGN.md
// section 5.23): per plane of a [Z, X, Y] slab the counts and the fp64 sums of the absolute first differences along z, x and y and of the
// absolute second difference along z, over the voxel pairs (triples) that lie inside an optional mask.  Slice-wise synthesis leaves
// neighbouring planes without a common stochastic choice; that shows as a first difference along z that is large beside the in-plane ones.
//
// The reduction is the one of volume_metrics.hip: partials per (plane, workgroup) go to a workspace and a second kernel adds a plane's
// partials in workgroup order.  No atomics: the sums are the same bits on every run.
#include "volume_common.h"

#define TP_THREADS 256
#define TP_WAVES (TP_THREADS / 64)
#define TP_PARTS MUD_TP_PARTS
#define TP_NQ MUD_TP_NQ

// workgroup (plane zi, part p): the voxels p * TP_THREADS + t, + TP_PARTS * TP_THREADS, ... of plane z0 + zi.  A voxel inside the mask adds
// |V[z+1] - V[z]| when the voxel above is inside too (and z < z1), |V[z+1] - 2 V[z] + V[z-1]| when the one below is as well (z > z0), and the
// differences to its +x and +y neighbours, all in fp64 from the fp32 values.  Every thread reaches both barriers.
__global__ __launch_bounds__(TP_THREADS) void k_volume_through_plane(const float* __restrict__ vol, const uint8_t* __restrict__ mask, int X, int Y,
                                                                    int z0, int z1, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[TP_WAVES][TP_NQ];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int p = blockIdx.x % TP_PARTS, zi = blockIdx.x / TP_PARTS;
  const int z = z0 + zi;
  const int64_t plane = (int64_t)X * Y;
  const float* v = vol + (int64_t)z * plane;
  const uint8_t* m = mask ? mask + (int64_t)z * plane : nullptr;
  const bool up = z < z1, down = z > z0;                                // uniform over the workgroup
  double acc[TP_NQ];
#pragma unroll
  for (int q = 0; q < TP_NQ; ++q) acc[q] = 0.0;
  for (int64_t i = (int64_t)p * TP_THREADS + t; i < plane; i += (int64_t)TP_PARTS * TP_THREADS) {
    if (m && !m[i]) continue;
    const int x = (int)(i / Y), y = (int)(i - (int64_t)x * Y);
    const double c = (double)v[i];
    const bool in_up = up && (!m || m[i + plane]), in_down = down && (!m || m[i - plane]);
    double a = 0.0;
    if (in_up) {
      a = (double)v[i + plane];
      acc[MUD_TP_N_DZ] += 1.0;
      acc[MUD_TP_S_DZ] += fabs(a - c);
    }
    if (in_up && in_down) {
      const double b = (double)v[i - plane];
      acc[MUD_TP_N_DZZ] += 1.0;
      acc[MUD_TP_S_DZZ] += fabs((a - 2.0 * c) + b);
    }
    if (x + 1 < X && (!m || m[i + Y])) {
      acc[MUD_TP_N_DX] += 1.0;
      acc[MUD_TP_S_DX] += fabs((double)v[i + Y] - c);
    }
    if (y + 1 < Y && (!m || m[i + 1])) {
      acc[MUD_TP_N_DY] += 1.0;
      acc[MUD_TP_S_DY] += fabs((double)v[i + 1] - c);
    }
  }
#pragma unroll
  for (int q = 0; q < TP_NQ; ++q) {
    const double s = mud_wave_sum(acc[q]);
    if (lane == 0) red[wave][q] = s;
  }
  __syncthreads();
  if (t < TP_NQ) {
    double s = 0.0;
#pragma unroll
    for (int wv = 0; wv < TP_WAVES; ++wv) s += red[wv][t];
    part[((int64_t)zi * TP_PARTS + p) * TP_NQ + t] = s;
  }
}

// one lane per (plane, quantity): the plane's partials in workgroup order
__global__ __launch_bounds__(TP_THREADS) void k_volume_through_plane_final(const double* __restrict__ part, int64_t n, double* __restrict__ sums) {
  const int64_t i = (int64_t)blockIdx.x * TP_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t zi = i / TP_NQ, q = i - zi * TP_NQ;
  double s = 0.0;
  for (int k = 0; k < TP_PARTS; ++k) s += part[(zi * TP_PARTS + k) * TP_NQ + q];
  sums[i] = s;
}

extern "C" int mud_volume_through_plane(const float* vol, const uint8_t* mask, int Z, int X, int Y, int z0, int z1, double* sums, void* ws,
                                        int64_t ws_bytes, void* stream) {
  if (int e = vi_check_size("mud_volume_through_plane", "volume", X, Y, Z)) return e;
  MUD_REQUIRE(z0 >= 0 && z0 <= z1 && z1 < Z, "mud_volume_through_plane: planes %d..%d are not a range of the %d planes", z0, z1, Z);
  MUD_REQUIRE(vol && sums && ws, "mud_volume_through_plane: null pointer");
  const int64_t planes = (int64_t)z1 - z0 + 1, need = planes * TP_PARTS * TP_NQ * 8;
  MUD_REQUIRE(ws_bytes >= need, "mud_volume_through_plane: ws holds %lld bytes, needs %lld", (long long)ws_bytes, (long long)need);
  MUD_REQUIRE(vi_aligned(ws, 8) && vi_aligned(sums, 8) && vi_aligned(vol, 4), "mud_volume_through_plane: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_volume_through_plane, dim3((unsigned)(planes * TP_PARTS)), dim3(TP_THREADS), 0, st, vol, mask, X, Y, z0, z1, (double*)ws);
  hipLaunchKernelGGL(k_volume_through_plane_final, dim3((unsigned)mud_cdiv(planes * TP_NQ, TP_THREADS)), dim3(TP_THREADS), 0, st,
                     (const double*)ws, planes * TP_NQ, sums);
  MUD_CHECK_LAUNCH("mud_volume_through_plane");
  return MUD_OK;
}
