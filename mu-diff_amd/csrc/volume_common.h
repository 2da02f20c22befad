// What the kernels of the volume pipeline share (volume_intake.hip, volume_coreg.hip, volume_bias.hip): the value of a stored voxel, the trilinear value
// at a source coordinate, the datatype dispatch and the argument checks of a stored volume.  One definition each, so that a histogram
// sample of mud_volume_joint_hist is the voxel mud_volume_regrid writes, bit for bit.
#pragma once
#include "mud_common.h"

#define VI_THREADS 256
#define VI_MAX_BLOCKS 2048

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
__device__ __forceinline__ float vi_trilinear(const T* __restrict__ src, int SX, int SY, int SZ, int scaled, double slope, double inter,
                                              const double p[3]) {
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
      acc = fma((double)vi_value<T>(src[((int64_t)zz * SY + yy) * SX + xx], scaled, slope, inter), w, acc);
  }
  return (float)acc;
}

// ---- shared by the histograms of volume_coreg.hip and volume_bias.hip: the bin of a value, a stored voxel by datatype code, finiteness
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

__device__ __forceinline__ float vc_stored_value(const void* __restrict__ p, int datatype, int64_t i, int scaled, double slope, double inter) {
  switch (datatype) {                          // uniform over the launch
    case MUD_NIFTI_U1: return vi_value<uint8_t>(((const uint8_t*)p)[i], scaled, slope, inter);
    case MUD_NIFTI_I2: return vi_value<int16_t>(((const int16_t*)p)[i], scaled, slope, inter);
    case MUD_NIFTI_U2: return vi_value<uint16_t>(((const uint16_t*)p)[i], scaled, slope, inter);
    case MUD_NIFTI_I4: return vi_value<int32_t>(((const int32_t*)p)[i], scaled, slope, inter);
    default: return vi_value<float>(((const float*)p)[i], scaled, slope, inter);
  }
}

__device__ __forceinline__ bool vc_finite(float v) { return fabsf(v) <= 3.402823466e38f; }

static inline bool vi_scaled(float slope, float inter) {      // volume.read_nifti's condition
  return slope != 0.0f && slope - slope == 0.0f && (slope != 1.0f || inter != 0.0f);
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

static inline int vi_check_volume(const char* who, const void* vol, int datatype, int X, int Y, int Z) {
  MUD_REQUIRE(vi_esize(datatype) != 0, "%s: unsupported NIfTI datatype code %d (u1 2, i2 4, i4 8, f4 16, u2 512)", who, datatype);
  MUD_REQUIRE(X > 0 && Y > 0 && Z > 0 && (int64_t)X * Y * Z < ((int64_t)1 << 31), "%s: bad volume size %d x %d x %d", who, X, Y, Z);
  MUD_REQUIRE(vol != nullptr, "%s: null pointer", who);
  MUD_REQUIRE(mud_aligned16(vol), "%s: the volume must be 16-byte aligned", who);
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
