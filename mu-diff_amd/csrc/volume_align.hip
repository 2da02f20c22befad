// Mid-sagittal alignment of the volume pipeline's inputs (--align; include/mudiff_hip.h: mud_volume_mirror_moments;
// mudiff_hip.volume_align).
//
// The search for the plane about which a head best matches its own mirror image runs on the host; what it evaluates, thousands of times
// per subject, is the correlation of the volume with its mirror image through a candidate plane.  One launch scores K candidates: the
// host hands over, per candidate, the matrix that maps a voxel index to the voxel coordinate of its mirror image, and the kernel returns
// per candidate the six integer sums n, sum a, sum b, sum a^2, sum b^2, sum a b of the bin indices a (the voxel) and b (the trilinear value
// at the mirrored coordinate, volume_common.h's rule: the voxel mud_volume_regrid would write there) over the overlap.  The Pearson
// correlation follows on the host in fp64.  Integer sums, as in volume_coreg.hip: the result does not depend on the order of arrival.
//
// The shape: a workgroup owns VA_POINTS x VI_THREADS consecutive sample points (x fastest, so that a wave's voxels are a run along x
// and their mirror images a run along the mirrored x) and `chunk` <= VA_CHUNK candidates (blockIdx.y; the entry point picks the chunk:
// VA_CHUNK when there is work for every CU anyway, fewer when K x the sample points are few, so that a refinement level of 27
// candidates at a coarse stride still fills the chip - integer sums do not depend on the split).  A thread reads its VA_POINTS voxels and
// bins them once, keeps them in registers, and loops over the workgroup's candidates: the matrix of one candidate is 12 wave-uniform
// loads, never 12 K registers.  Per candidate the six sums are formed in registers (uint32: at most 8 points x 255^2 per thread, 64 times
// that per wave), added across the wave by shuffles and left in LDS; after the last candidate one thread per (candidate, sum) adds the
// waves' parts and issues one 64-bit atomic add, 6 consecutive uint64 per candidate, and none for a sum of 0.
#include "volume_common.h"

#define VA_MAX_BINS 256
#define VA_POINTS 8                            // sample points per thread
#define VA_CHUNK 16                            // candidates per workgroup, at most
#define VA_FILL 1024                           // workgroups that fill an MI355X once: its 256 CUs x 4 resident workgroups of 4 waves (another
                                               // part would want its own figure; the result does not depend on it, only the launch shape)
#define VA_WAVES (VI_THREADS / 64)
#define VA_MAX_K (65535 * VA_CHUNK)            // gridDim.y at the full chunk

__device__ __forceinline__ uint32_t va_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_va_mirror_moments(vi_source src, int X, int Y, int Z, const double* __restrict__ mats, int K, int chunk, int stride,
                                                                  int nx, int ny, int64_t n, double lo, double scale, int bins,
                                                                  unsigned long long* __restrict__ sums) {
  __shared__ uint32_t part[VA_CHUNK * 6 * VA_WAVES];      // [candidate][sum][wave]
  int px[VA_POINTS], py[VA_POINTS], pz[VA_POINTS], pa[VA_POINTS];      // the thread's sample points and their bins; -1: not a sample
  const int64_t first = (int64_t)blockIdx.x * (VI_THREADS * VA_POINTS) + threadIdx.x;
#pragma unroll
  for (int j = 0; j < VA_POINTS; ++j) {
    const int64_t i = first + (int64_t)j * VI_THREADS;
    px[j] = py[j] = pz[j] = 0, pa[j] = -1;
    if (i < n) {
      int xi, yj, zk;
      vi_xyz(i, nx, ny, xi, yj, zk);
      px[j] = xi * stride, py[j] = yj * stride, pz[j] = zk * stride;
      const float v = vi_at<T>(src, ((int64_t)pz[j] * Y + py[j]) * X + px[j]);
      if (vc_finite(v)) pa[j] = vc_bin(v, lo, scale, bins);
    }
  }
  const int k0 = (int)blockIdx.y * chunk;                // chunk: 1 .. VA_CHUNK
  const int kc = K - k0 < chunk ? K - k0 : chunk;        // >= 1 by the launch shape
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = 0; c < kc; ++c) {
    vi_mat M;                                  // wave-uniform: blockIdx and the loop counter only
#pragma unroll
    for (int i = 0; i < 12; ++i) M.m[i] = mats[(int64_t)(k0 + c) * 12 + i];
    uint32_t s[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < VA_POINTS; ++j) {
      if (pa[j] < 0) continue;
      double p[3];
      vi_coordinate(M, (double)px[j], (double)py[j], (double)pz[j], p);
      // the overlap: 0 <= p <= S - 1 on every axis (a NaN fails); inside it every neighbour of non-zero weight is a stored voxel
      if (!(p[0] >= 0.0 && p[0] <= (double)(X - 1) && p[1] >= 0.0 && p[1] <= (double)(Y - 1) && p[2] >= 0.0 && p[2] <= (double)(Z - 1))) continue;
      const float mv = vi_trilinear<T>(src, X, Y, Z, p);
      if (!vc_finite(mv)) continue;
      const uint32_t a = (uint32_t)pa[j], b = (uint32_t)vc_bin(mv, lo, scale, bins);
      s[0] += 1u, s[1] += a, s[2] += b, s[3] += a * a, s[4] += b * b, s[5] += a * b;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const uint32_t t = va_wave_sum(s[q]);
      if (lane == 0) part[(c * 6 + q) * VA_WAVES + wave] = t;
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < kc * 6; t += VI_THREADS) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < VA_WAVES; ++w) total += part[t * VA_WAVES + w];
    if (total) atomicAdd(&sums[(int64_t)k0 * 6 + t], total);
  }
}

extern "C" int mud_volume_mirror_moments(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, const double* mats, int K,
                                         int stride, double lo, double scale, int bins, uint64_t* sums, void* stream) {
  if (int e = vi_check_volume("mud_volume_mirror_moments", vol, datatype, X, Y, Z)) return e;
  MUD_REQUIRE(mats != nullptr && sums != nullptr, "mud_volume_mirror_moments: null pointer");
  MUD_REQUIRE(vi_aligned(mats, 8) && vi_aligned(sums, 8), "mud_volume_mirror_moments: mats and sums must be 8-byte aligned");
  MUD_REQUIRE(K >= 1 && K <= VA_MAX_K, "mud_volume_mirror_moments: 1 to %d candidates, got %d", VA_MAX_K, K);
  MUD_REQUIRE(stride > 0, "mud_volume_mirror_moments: stride %d is not positive", stride);
  if (int e = vi_check_bins("mud_volume_mirror_moments", lo, scale, bins, 2, VA_MAX_BINS)) return e;
  hipStream_t s = (hipStream_t)stream;
  const int nx = (int)mud_cdiv(X, stride), ny = (int)mud_cdiv(Y, stride), nz = (int)mud_cdiv(Z, stride);
  const int64_t n = (int64_t)nx * ny * nz;
  const vi_source v = vi_source_of(vol, datatype, slope, inter);
  const int64_t tiles = mud_cdiv(n, (int64_t)VI_THREADS * VA_POINTS);
  const int64_t fill = mud_cdiv(tiles * K, VA_FILL);     // candidates per workgroup at which the launch has VA_FILL workgroups
  const int chunk = (int)(fill < 1 ? 1 : fill > VA_CHUNK ? VA_CHUNK : fill);      // (a chunk below VA_CHUNK means K <= 16 VA_FILL: gridDim.y fits)
  if (int e = vi_clear("mud_volume_mirror_moments", sums, sizeof(uint64_t) * 6 * (size_t)K, s)) return e;
  const dim3 grid((unsigned)tiles, (unsigned)mud_cdiv(K, chunk));
  VI_DISPATCH(datatype, hipLaunchKernelGGL(k_va_mirror_moments<T>, grid, dim3(VI_THREADS), 0, s, v, X, Y, Z, mats, K, chunk, stride, nx, ny, n, lo, scale,
                                           bins, (unsigned long long*)sums));
  MUD_CHECK_LAUNCH("mud_volume_mirror_moments");
  return MUD_OK;
}
