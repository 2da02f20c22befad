// What the kernels of the volume pipeline share (volume_intake.hip, volume_coreg.hip, volume_bias.hip, volume_denoise.hip,
// volume_foreground.hip): a stored volume as one kernel argument and the value of its voxels, the trilinear value at a source coordinate,
// the order-preserving key, the index and loop helpers, the LDS histogram and the per-workgroup count, the launch shapes and the argument
// checks.  One definition each, so that a histogram sample of mud_volume_joint_hist is the voxel mud_volume_regrid writes and a key decodes
// to the value that was encoded, bit for bit.  DESIGN.md section 5.17 lists them.
#pragma once
#include "mud_common.h"

#define VI_THREADS 256
#define VI_MAX_BLOCKS 2048
#define VI_TX 32                               // the tile of the kernels that stage a neighbourhood in LDS (denoise, foreground)
#define VI_TY 8
#define VI_TZ 4

// the grid-stride loop of a one-dimensional launch of VI_THREADS threads per workgroup
#define VI_GRID_STRIDE(i, n) for (int64_t i = (int64_t)blockIdx.x * VI_THREADS + threadIdx.x; i < (n); i += (int64_t)gridDim.x * VI_THREADS)

// ---- the value of a stored voxel ------------------------------------------------------------------------------------------------------
// float32(double(raw) * slope + inter), the product and the sum rounded separately (numpy: data.astype(float64) * slope + inter, then
// astype(float32)); without scaling float32(double(raw)) = float32(raw)
template <typename T>
__device__ __forceinline__ float vi_value(T raw, int scaled, double slope, double inter) {
#pragma clang fp contract(off)
  double d = (double)raw;
  if (scaled) {
    d = d * slope;
    d = d + inter;
  }
  return (float)d;
}

static inline bool vi_scaled(float slope, float inter) {      // volume.read_nifti's condition
  return slope != 0.0f && slope - slope == 0.0f && (slope != 1.0f || inter != 0.0f);
}

struct vi_source {                             // a stored volume as a kernel argument: the voxels as the file holds them and how to read them
  const void* vol;
  int datatype, scaled;
  double slope, inter;
};

static inline vi_source vi_source_of(const void* vol, int datatype, float slope, float inter) {
  return {vol, datatype, (int)vi_scaled(slope, inter), (double)slope, (double)inter};
}

template <typename T>                          // voxel i of a volume whose datatype is T (VI_DISPATCH)
__device__ __forceinline__ float vi_at(const vi_source& s, int64_t i) {
  return vi_value<T>(((const T*)s.vol)[i], s.scaled, s.slope, s.inter);
}

__device__ __forceinline__ float vc_stored_value(const vi_source& s, int64_t i) {      // voxel i by the datatype code
  switch (s.datatype) {                        // uniform over the launch
    case MUD_NIFTI_U1: return vi_at<uint8_t>(s, i);
    case MUD_NIFTI_I2: return vi_at<int16_t>(s, i);
    case MUD_NIFTI_U2: return vi_at<uint16_t>(s, i);
    case MUD_NIFTI_I4: return vi_at<int32_t>(s, i);
    default: return vi_at<float>(s, i);
  }
}

// m maps a reference voxel index (i, j, k) to a source voxel coordinate p; everything about p is fp64, so that an identity, an integer
// shift, a flip or a dyadic scale reproduce stored values exactly and an oblique matrix places a 240-voxel axis to ~1e-13 voxels.
struct vi_mat {
  double m[12];
};

__device__ __forceinline__ void vi_coordinate(const vi_mat& M, double x, double y, double z, double p[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = fma(M.m[4 * a], x, fma(M.m[4 * a + 1], y, fma(M.m[4 * a + 2], z, M.m[4 * a + 3])));
}

// one axis of p: is any neighbour inside [0, S)?  With p in (-1, S) floor(p) fits an int; a NaN or an infinite p fails the test
__device__ __forceinline__ bool vi_axis_near(double p, int S) { return p > -1.0 && p < (double)S; }

// the trilinear value at p (vi_axis_near on every axis): the fp64 sum over the 8 neighbours, rounded to fp32 once
template <typename T>
__device__ __forceinline__ float vi_trilinear(const vi_source& src, int SX, int SY, int SZ, const double p[3]) {
  const double fx = floor(p[0]), fy = floor(p[1]), fz = floor(p[2]);
  const double wx[2] = {1.0 - (p[0] - fx), p[0] - fx}, wy[2] = {1.0 - (p[1] - fy), p[1] - fy}, wz[2] = {1.0 - (p[2] - fz), p[2] - fz};
  const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
  double acc = 0.0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {                          // neighbours in file order: x fastest
    const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
    const int xx = x0 + dx, yy = y0 + dy, zz = z0 + dz;
    const double w = wx[dx] * wy[dy] * wz[dz];
    // a neighbour of weight 0 is not read (an identity next to a NaN stays exact); one outside the grid counts as 0
    if (w != 0.0 && xx >= 0 && xx < SX && yy >= 0 && yy < SY && zz >= 0 && zz < SZ)
      acc = fma((double)vi_at<T>(src, ((int64_t)zz * SY + yy) * SX + xx), w, acc);
  }
  return (float)acc;
}

// ---- packed reads of sub-dword voxels (volume_reorient.hip, volume_lowpass.hip) ----------------------------------------------------------
// a word of sizeof(W) / sizeof(T) elements from an address of unknown alignment (rows of a volume start where they start; gfx950 global
// memory takes it as one access), and element k of it
template <typename W, typename T>
__device__ __forceinline__ W vo_load(const T* p) {
  W w;
  __builtin_memcpy(&w, p, sizeof(W));
  return w;
}
template <typename T, typename W>             // element k of a word (little-endian: the element at the lower address first)
__device__ __forceinline__ T vo_element(W w, int k) { return (T)(w >> (8 * sizeof(T) * k)); }

// ---- keys, bins and indices -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool vc_finite(float v) { return fabsf(v) <= 3.402823466e38f; }

// order-preserving uint32 image of an fp32 that is not a NaN: unsigned comparison of keys = comparison of values
__device__ __forceinline__ uint32_t vc_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the same with every NaN sorting last (np.sort puts them there), and its inverse
__device__ __forceinline__ uint32_t vi_key(float v) { return v != v ? 0xFFFFFFFFu : vc_key(v); }
__device__ __forceinline__ float vi_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// clamp((int)floor((double(v) - lo) * scale), 0, bins - 1), the subtraction and the product rounded separately (numpy's two steps);
// clamped before the conversion, so that no product is too large for an int
__device__ __forceinline__ int vc_bin(float v, double lo, double scale, int bins) {
#pragma clang fp contract(off)
  double d = (double)v - lo;
  d = d * scale;
  d = floor(d);
  const double top = (double)(bins - 1);
  d = d > 0.0 ? d : 0.0;
  d = d < top ? d : top;
  return (int)d;
}

// linear index i of a grid with X x Y voxels per plane -> (x, y, z) by two 32-bit divisions: i < 2^31, because every entry point
// refuses a volume of 2^31 voxels or more (vi_check_size).  A strided sample grid passes (nx, ny) and multiplies by its stride.
__device__ __forceinline__ void vi_xyz(int64_t i, int X, int Y, int& x, int& y, int& z) {
  const uint32_t l = (uint32_t)i;
  const uint32_t row = l / (uint32_t)X;
  x = (int)(l - row * (uint32_t)X), y = (int)(row % (uint32_t)Y), z = (int)(row / (uint32_t)Y);
}

// ---- the LDS-privatised histogram: vc_hist_clear, count into h[] with LDS atomics, vc_hist_merge (one global atomic per non-empty bin).
// A workgroup's count of something is the histogram of one bin: vc_hist_clear(&s, 1), if (mine) atomicAdd(&s, mine), vc_hist_merge(&s, 1, total).
// Both contain a barrier: every thread of the workgroup must reach them, so no thread may return before the merge.
__device__ __forceinline__ void vc_hist_clear(uint32_t* h, int nb) {
  for (int i = threadIdx.x; i < nb; i += VI_THREADS) h[i] = 0;
  __syncthreads();
}
__device__ __forceinline__ void vc_hist_merge(const uint32_t* h, int nb, uint32_t* __restrict__ hist) {
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += VI_THREADS) {
    const uint32_t c = h[i];
    if (c) atomicAdd(&hist[i], c);
  }
}

// ---- host side: launch shapes and argument checks ---------------------------------------------------------------------------------------
// the workgroups of a grid-stride launch: clamp(cdiv(n, per_block), 1, cap)
static inline unsigned vi_blocks(int64_t n, int64_t per_block = VI_THREADS, int64_t cap = VI_MAX_BLOCKS) {
  const int64_t b = mud_cdiv(n, per_block);
  return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

static inline dim3 vi_tile_grid(int X, int Y, int Z) {
  return dim3((unsigned)mud_cdiv(X, VI_TX), (unsigned)mud_cdiv(Y, VI_TY), (unsigned)mud_cdiv(Z, VI_TZ));
}

static inline bool vi_aligned(const void* p, size_t bytes) { return (((uintptr_t)p) & (uintptr_t)(bytes - 1)) == 0; }      // bytes: a power of two

// fill `bytes` at p on the stream (with zeros unless told otherwise) before the kernels that accumulate into it
static inline int vi_clear(const char* who, void* p, size_t bytes, hipStream_t s, int fill = 0) {
  if (hipMemsetAsync(p, fill, bytes, s) != hipSuccess) {
    mud_set_error("%s: clearing the result failed", who);
    return MUD_ERR_LAUNCH;
  }
  return MUD_OK;
}

// dynamic LDS above the default limit of a launch has to be allowed per kernel and device
static inline int vi_allow_lds(const char* who, mud_attr_once& once, const void* kernel, int bytes) {
  if (once.need()) {
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
      mud_set_error("%s: cannot reserve %d B of LDS: %s", who, bytes, hipGetErrorString(e));
      return MUD_ERR_LAUNCH;
    }
    once.ok();
  }
  return MUD_OK;
}

static inline int vi_esize(int datatype) {
  switch (datatype) {
    case MUD_NIFTI_U1: return 1;
    case MUD_NIFTI_I2:
    case MUD_NIFTI_U2: return 2;
    case MUD_NIFTI_I4:
    case MUD_NIFTI_F4: return 4;
    default: return 0;
  }
}

// fewer than 2^31 voxels: what lets every kernel index with 32-bit divisions (vi_xyz) and an int label hold a linear index
static inline int vi_check_size(const char* who, const char* what, int X, int Y, int Z) {
  MUD_REQUIRE(X > 0 && Y > 0 && Z > 0 && (int64_t)X * Y * Z < ((int64_t)1 << 31), "%s: bad %s size %d x %d x %d", who, what, X, Y, Z);
  return MUD_OK;
}

static inline int vi_check_volume(const char* who, const void* vol, int datatype, int X, int Y, int Z) {
  MUD_REQUIRE(vi_esize(datatype) != 0, "%s: unsupported NIfTI datatype code %d (u1 2, i2 4, i4 8, f4 16, u2 512)", who, datatype);
  if (int e = vi_check_size(who, "volume", X, Y, Z)) return e;
  MUD_REQUIRE(vol != nullptr, "%s: null pointer", who);
  MUD_REQUIRE(mud_aligned16(vol), "%s: the volume must be 16-byte aligned", who);
  return MUD_OK;
}

// a grid of VI_TX x VI_TY x VI_TZ tiles (vi_tile_grid) has at most 65535 workgroups along y and z
static inline int vi_check_tiled(const char* who, int X, int Y, int Z) {
  MUD_REQUIRE(Y <= VI_TY * 65535 && Z <= VI_TZ * 65535, "%s: bad volume size %d x %d x %d", who, X, Y, Z);
  return MUD_OK;
}

static inline int vi_check_bins(const char* who, double lo, double scale, int bins, int min_bins, int max_bins) {
  MUD_REQUIRE(bins >= min_bins && bins <= max_bins, "%s: %d to %d bins, got %d", who, min_bins, max_bins, bins);
  MUD_REQUIRE(lo - lo == 0.0 && scale - scale == 0.0, "%s: lo / scale must be finite (%g, %g)", who, lo, scale);
  return MUD_OK;
}

#define VI_DISPATCH(datatype, CALL)                           \
  switch (datatype) {                                         \
    case MUD_NIFTI_U1: { typedef uint8_t T; CALL; } break;    \
    case MUD_NIFTI_I2: { typedef int16_t T; CALL; } break;    \
    case MUD_NIFTI_U2: { typedef uint16_t T; CALL; } break;   \
    case MUD_NIFTI_I4: { typedef int32_t T; CALL; } break;    \
    default: { typedef float T; CALL; } break;                \
  }
