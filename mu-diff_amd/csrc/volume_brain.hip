// Brain extraction of the volume pipeline's inputs (--brain_extract; include/mudiff_hip.h: mud_volume_edt*; mudiff_hip.volume_brain;
// DESIGN.md section 5.18): morphology by a radius in millimetres on an anisotropic grid, which is a threshold on an exact Euclidean
// distance transform.  The rest of the extraction (threshold, largest component, holes) is volume_foreground.hip's.
//
// The definition of mud_volume_edt, bit for bit.  wx = sx * sx, wy = sy * sy, wz = sz * sz, each rounded once.  For a voxel p and every
// voxel q of the volume whose mask equals `value`, with the integer offsets (dx, dy, dz) = q - p, every product and every sum rounded
// separately (no fused multiply-add):
//     d2[p] = min over q of ((wx * (dx * dx)) + (wy * (dy * dy))) + (wz * (dz * dz))           (+inf without any q)
// dx * dx is an exact integer.  fp64 addition is monotone (a <= b implies fl(a + c) <= fl(b + c)), so the minimum over q of a rounded
// sum is the rounded sum of the minimum, and the definition separates exactly into three passes of one line operation,
//     out(i) = min over j of (in(j) + w * ((i - j) * (i - j))),
// along x (in = 0 at a voxel whose mask equals `value`, +inf elsewhere), then y, then z, each in place on d2.  The line operation is a
// plain scan that walks away from i in both directions and stops once w * k^2 is not below the best value so far: in(j) >= 0, so no
// later term can be smaller, and the work per voxel is bounded by the distance found, not by the length of the line.
//
// One kernel serves the three passes.  A workgroup stages a slab of whole lines in LDS as [slow][fast] with `fast` contiguous in memory:
// for the x pass the lines themselves (fast = the position on the line, slow = the line), for the y and z passes a run of adjacent
// x (for z: of adjacent x + X * y) of every position of the line (fast = the column, slow = the position), so that every global read and
// write is a run of consecutive addresses and consecutive lanes touch consecutive LDS words while they scan.  No floating-point atomics,
// no order that depends on the launch: two runs give the same bits.
#include <cmath>
#include "volume_common.h"

#define EDT_MAX_LINE 1024                      // the longest axis: a line is staged whole
#define EDT_SLAB 8192                          // fp64 values of a slab: 64 KiB of LDS
#define EDT_MIN_COLS 8                         // columns of a y / z slab: EDT_SLAB / EDT_MAX_LINE at the least, 256 at the most
#define EDT_MAX_COLS 256
#define EDT_ROWS_SLAB 4096                     // values of an x slab: as many whole rows as fit (one at the least)

static_assert(EDT_MIN_COLS * EDT_MAX_LINE <= EDT_SLAB && EDT_MAX_LINE <= EDT_ROWS_SLAB && EDT_ROWS_SLAB <= EDT_SLAB, "a slab fits the LDS");

struct edt_pass {                              // one pass: the volume as planes of [slow][fast] elements and how the workgroups tile it
  int64_t plane_stride, row_stride;            // elements between planes / between rows (slow + 1)
  int fast_total, slow_total;                  // the extent of a plane
  int fast_tile, slow_tile;                    // what a workgroup takes of it: fast_tile * slow_tile <= EDT_SLAB
  int fast_tiles, slow_tiles;                  // cdiv of the above
  int along;                                   // 1: the line runs along fast (x pass), 0: along slow (y and z passes); a tile spans the line
  double w;                                    // the squared spacing of the pass's axis
};

// out(i) of the line through LDS word p (position i of n, `step` words between positions)
__device__ __forceinline__ double edt_line_min(const double* s, int p, int step, int i, int n, double w) {
#pragma clang fp contract(off)
  double best = s[p];
  const int reach = i > n - 1 - i ? i : n - 1 - i;
  for (int k = 1; k <= reach; ++k) {
    const double wk = w * (double)(k * k);     // k <= 1023: k * k is exact in an int
    if (!(wk < best)) break;
    if (k <= i) {
      const double c = s[p - k * step] + wk;
      best = c < best ? c : best;
    }
    if (i + k < n) {
      const double c = s[p + k * step] + wk;
      best = c < best ? c : best;
    }
  }
  return best;
}

// mask != nullptr: the first pass, in(j) = 0 where the mask equals `value`, +inf elsewhere; else in = d2.  In place: a workgroup reads
// and writes its own lines only, and it has read them all (the barrier) before it writes one.
__global__ __launch_bounds__(VI_THREADS) void k_edt_pass(const uint8_t* __restrict__ mask, int value, double* d2, edt_pass g) {
  extern __shared__ double edt_s[];
  const int b = (int)blockIdx.x;
  const int ft = b % g.fast_tiles, r = b / g.fast_tiles, st = r % g.slow_tiles, plane = r / g.slow_tiles;
  const int f0 = ft * g.fast_tile, s0 = st * g.slow_tile;
  const int nf = min(g.fast_tile, g.fast_total - f0), ns = min(g.slow_tile, g.slow_total - s0);
  const int count = nf * ns;                   // <= fast_tile * slow_tile <= EDT_SLAB
  const int64_t base = (int64_t)plane * g.plane_stride + (int64_t)s0 * g.row_stride + f0;
  const bool on = value != 0;
  for (int idx = threadIdx.x; idx < count; idx += VI_THREADS) {
    const int slow = idx / nf, fast = idx - slow * nf;
    const int64_t a = base + (int64_t)slow * g.row_stride + fast;
    edt_s[idx] = mask != nullptr ? (((mask[a] != 0) == on) ? 0.0 : (double)INFINITY) : d2[a];
  }
  __syncthreads();
  const int step = g.along ? 1 : nf, n = g.along ? nf : ns;
  for (int idx = threadIdx.x; idx < count; idx += VI_THREADS) {
    const int slow = idx / nf, fast = idx - slow * nf;
    d2[base + (int64_t)slow * g.row_stride + fast] = edt_line_min(edt_s, idx, step, g.along ? fast : slow, n, g.w);
  }
}

// ---- out = (above ? d2 > r2 : d2 <= r2) and within; count: the voxels switched on
__global__ __launch_bounds__(VI_THREADS) void k_edt_select(const double* __restrict__ d2, int64_t n, double r2, int above,
                                                           const uint8_t* __restrict__ within, uint8_t* __restrict__ out,
                                                           uint32_t* __restrict__ count) {
  __shared__ uint32_t s;                       // the workgroup's count: a histogram of one bin
  vc_hist_clear(&s, 1);
  uint32_t mine = 0;
  VI_GRID_STRIDE(i, n) {
    const double d = d2[i];
    const bool keep = (above ? d > r2 : d <= r2) && (within == nullptr || within[i] != 0);
    out[i] = keep ? 1 : 0;
    mine += keep ? 1 : 0;
  }
  if (mine) atomicAdd(&s, mine);
  vc_hist_merge(&s, 1, count);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------
static inline int edt_floor_pow2(int v) {
  int p = 1;
  while (2 * p <= v) p *= 2;
  return p;
}

// the pass along `axis` (0: x, 1: y, 2: z) of an X x Y x Z volume
static inline edt_pass edt_pass_of(int axis, int X, int Y, int Z, double spacing) {
  edt_pass g;
  const int64_t XY = (int64_t)X * Y;
  if (axis == 0) {                             // rows of X: a slab is whole rows, next to each other in memory
    const int rows = EDT_ROWS_SLAB / X;
    g = {0, X, X, (int)((int64_t)Y * Z), X, rows < 1 ? 1 : rows, 1, 0, 1, 0.0};
  } else {
    const int L = axis == 1 ? Y : Z;
    int cols = edt_floor_pow2(EDT_SLAB / L);
    cols = cols < EDT_MIN_COLS ? EDT_MIN_COLS : cols > EDT_MAX_COLS ? EDT_MAX_COLS : cols;
    if (axis == 1) g = {XY, X, X, Y, cols, Y, 0, 1, 0, 0.0};                    // a plane per z, columns = adjacent x
    else g = {0, XY, (int)XY, Z, cols, Z, 0, 1, 0, 0.0};                         // one plane, columns = adjacent x + X * y
  }
  g.fast_tiles = (int)mud_cdiv(g.fast_total, g.fast_tile);
  g.slow_tiles = (int)mud_cdiv(g.slow_total, g.slow_tile);
  g.w = spacing * spacing;
  return g;
}

extern "C" int mud_volume_edt(const uint8_t* mask, int X, int Y, int Z, int value, double sx, double sy, double sz, double* d2, void* stream) {
  if (int e = vi_check_size("mud_volume_edt", "volume", X, Y, Z)) return e;
  MUD_REQUIRE(X <= EDT_MAX_LINE && Y <= EDT_MAX_LINE && Z <= EDT_MAX_LINE,
              "mud_volume_edt: an axis of %d x %d x %d is longer than the %d voxels of a staged line", X, Y, Z, EDT_MAX_LINE);
  MUD_REQUIRE(value == 0 || value == 1, "mud_volume_edt: the value to measure the distance to must be 0 or 1 (got %d)", value);
  MUD_REQUIRE(sx - sx == 0.0 && sy - sy == 0.0 && sz - sz == 0.0 && sx > 0.0 && sy > 0.0 && sz > 0.0,
              "mud_volume_edt: the spacing must be finite and > 0 (got %g, %g, %g)", sx, sy, sz);
  MUD_REQUIRE(mask != nullptr && d2 != nullptr, "mud_volume_edt: null pointer");
  MUD_REQUIRE(mud_aligned16(d2), "mud_volume_edt: d2 must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const double spacing[3] = {sx, sy, sz};
  for (int axis = 0; axis < 3; ++axis) {
    const edt_pass g = edt_pass_of(axis, X, Y, Z, spacing[axis]);
    const int64_t planes = axis == 1 ? Z : 1;
    const int64_t blocks = planes * g.slow_tiles * g.fast_tiles;               // < 2^31: fewer than the voxels
    const size_t lds = sizeof(double) * (size_t)g.fast_tile * (size_t)g.slow_tile;
    hipLaunchKernelGGL(k_edt_pass, dim3((unsigned)blocks), dim3(VI_THREADS), lds, s, axis == 0 ? mask : (const uint8_t*)nullptr, value, d2, g);
  }
  MUD_CHECK_LAUNCH("mud_volume_edt");
  return MUD_OK;
}

extern "C" int mud_volume_edt_select(const double* d2, int64_t n, double r2, int above, const uint8_t* within, uint8_t* out, uint32_t* count,
                                     void* stream) {
  MUD_REQUIRE(n > 0 && n < ((int64_t)1 << 31), "mud_volume_edt_select: bad voxel count %lld", (long long)n);
  MUD_REQUIRE(r2 - r2 == 0.0 && r2 >= 0.0, "mud_volume_edt_select: r2 must be finite and >= 0 (got %g)", r2);
  MUD_REQUIRE(above == 0 || above == 1, "mud_volume_edt_select: above must be 0 or 1 (got %d)", above);
  MUD_REQUIRE(d2 != nullptr && out != nullptr && count != nullptr, "mud_volume_edt_select: null pointer");
  MUD_REQUIRE(vi_aligned(d2, 8) && vi_aligned(count, 4), "mud_volume_edt_select: d2 must be 8-byte aligned, count 4-byte aligned");
  MUD_REQUIRE(out != within, "mud_volume_edt_select: out must be a buffer of its own");
  hipStream_t s = (hipStream_t)stream;
  if (int e = vi_clear("mud_volume_edt_select", count, sizeof(uint32_t), s)) return e;
  hipLaunchKernelGGL(k_edt_select, dim3(vi_blocks(n)), dim3(VI_THREADS), 0, s, d2, n, r2, above, within, out, count);
  MUD_CHECK_LAUNCH("mud_volume_edt_select");
  return MUD_OK;
}
