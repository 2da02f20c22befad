// Reorientation of a stored volume (--reorient; include/mudiff_hip.h: mud_volume_reorient; mudiff_hip.volume_reorient; DESIGN.md
// section 5.20): a permutation and flips of the storage axes, dst[i0,i1,i2] = src[j] with j[p_o] = flip_o ? S[p_o] - 1 - i_o : i_o.
// A pure move of 1-, 2-, 4- or 8-byte elements, x fastest on both sides; no arithmetic on the values, so every stored datatype, the
// fp32 volumes of the other stages and fp64 go through one template on the element width.
//
// Two access patterns:
//   p0 == 0  (k_vo_rows)   the fast axis stays the fast axis: whole x-rows are copied, read backwards under an x flip.  A thread moves one
//            dword (qword for 8-byte elements) of the destination: 64 lanes write 256 (512) contiguous bytes and read as many.
//   p0 != 0  (k_vo_tiles)  the source's fast axis becomes the destination's axis a (p_a = 0) and the source's axis p0 becomes the
//            destination's fast axis: a square tile of the plane (source x, source axis p0) goes through LDS.  It is read in runs along
//            source x and written in runs along destination x, 32 lanes x one dword (qword) = 128 (256) contiguous bytes either way,
//            whatever the element width: the tile is 32 * V elements on a side, V = elements per dword, so that sub-dword elements
//            travel packed on both sides of the LDS.  A workgroup takes one tile of one plane at a time and strides over the rest.
//
// The tile in LDS is kept in the destination's orientation (row = destination axis a, column = destination x; the flips are applied
// on the way in), V rows to a group: row r starts at dword (r / V) * (V * ROWD + PAD) + (r % V) * ROWD, ROWD = dwords per row, PAD = 1
// dword (2 for 8-byte elements, which keeps them 8-byte aligned).  On the way in the 32 lanes of a half-wave hold one source row:
// V * l + k -> row group l (or 31 - l), a stride of V * ROWD + PAD = PAD (mod 32) dwords: 32 different banks (16 bank pairs twice for
// 8-byte elements).  On the way out a half-wave reads the 32 consecutive dwords (qwords) of one row.
//
// Rows of a volume start where they start: a run of V sub-dword elements is not dword-aligned in global memory in general.  The packed
// accesses are therefore written as 4- / 8-byte copies of unknown alignment (gfx950 global memory takes them as one access); a run that
// crosses the end of a row falls back to single elements.
#include "volume_common.h"

#define VO_LANES 32                            // lanes along a run
#define VO_MAX_BLOCKS 16384                    // workgroups of a launch; the kernels stride over what is left

template <typename T> struct vo_word { typedef uint32_t W; };
template <> struct vo_word<uint64_t> { typedef uint64_t W; };

template <typename W, typename T>
__device__ __forceinline__ void vo_store(T* p, W w) { __builtin_memcpy(p, &w, sizeof(W)); }

template <typename T, typename W>             // the V elements of a word in reverse order
__device__ __forceinline__ W vo_reversed(W w) {
  if (sizeof(T) == 1) return (W)__builtin_bswap32((uint32_t)w);
  if (sizeof(T) == 2) return (W)(((uint32_t)w >> 16) | ((uint32_t)w << 16));
  return w;
}

// ---- p0 == 0: rows ------------------------------------------------------------------------------------------------------------------
struct vo_rows {
  int X, D1, S1;                               // the row length, the destination's second extent, the source's second extent
  int p1, fx, f1, f2;                          // p1: the source axis of destination axis 1 (1 or 2); the flips of the destination axes
  int D2;
};

__device__ __forceinline__ int64_t vo_src_row(const vo_rows& g, int i1, int i2) {
  const int u = g.f1 ? g.D1 - 1 - i1 : i1, v = g.f2 ? g.D2 - 1 - i2 : i2;
  const int s1 = g.p1 == 1 ? u : v, s2 = g.p1 == 1 ? v : u;
  return (int64_t)s2 * g.S1 + s1;
}

template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_vo_rows(const T* __restrict__ src, T* __restrict__ dst, vo_rows g, int64_t n, int64_t words) {
  typedef typename vo_word<T>::W W;
  constexpr int V = sizeof(W) / sizeof(T);
  VI_GRID_STRIDE(q, words) {
    const int64_t i = q * V;                   // the first destination element of this word
    int x, i1, i2;
    vi_xyz(i, g.X, g.D1, x, i1, i2);
    if (x + V <= g.X) {                        // the word lies inside one row (then i + V <= n too)
      const T* p = src + vo_src_row(g, i1, i2) * g.X + (g.fx ? g.X - V - x : x);
      W w = vo_load<W>(p);
      if (g.fx) w = vo_reversed<T, W>(w);
      vo_store<W>(dst + i, w);
    } else {
      for (int k = 0; k < V && i + k < n; ++k) {
        vi_xyz(i + k, g.X, g.D1, x, i1, i2);
        dst[i + k] = src[vo_src_row(g, i1, i2) * g.X + (g.fx ? g.X - 1 - x : x)];
      }
    }
  }
}

// ---- p0 != 0: tiles through LDS -----------------------------------------------------------------------------------------------------
struct vo_tiles {
  int S0, SP, ST;                              // the source's extents along x, along its axis p0 and along its third axis t
  int64_t sp_stride, st_stride;                // the source's strides, in elements, along p0 and t (x: 1)
  int64_t da_stride, db_stride;                // the destination's strides along a (p_a = 0) and b (p_b = t) (its x, which is source p0: 1)
  int f0, fa, fb;                              // the flips of the destination's x, a and b
  int tiles_x, tiles_y;
  int64_t total;                               // tiles_x * tiles_y * ST
};

template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_vo_tiles(const T* __restrict__ src, T* __restrict__ dst, vo_tiles g) {
  typedef typename vo_word<T>::W W;
  constexpr int E = sizeof(T), V = sizeof(W) / E, TILE = VO_LANES * V;
  constexpr int ROWD = TILE * E / 4, PAD = E == 8 ? 2 : 1, GROUP = V * ROWD + PAD;      // dwords
  __shared__ W lds[VO_LANES * GROUP * 4 / sizeof(W)];
  T* tile = (T*)lds;
  const int per_plane = g.tiles_x * g.tiles_y;
  for (int64_t work = blockIdx.x; work < g.total; work += gridDim.x) {
    const int st = (int)(work / per_plane), rem = (int)(work - (int64_t)st * per_plane);
    const int x0 = (rem % g.tiles_x) * TILE, y0 = (rem / g.tiles_x) * TILE;
    const T* from = src + st * g.st_stride;
    for (int q = threadIdx.x; q < TILE * VO_LANES; q += VI_THREADS) {      // in: runs along source x
      const int xl = V * (q % VO_LANES), yl = q / VO_LANES;
      const int sx = x0 + xl, sy = y0 + yl;
      if (sx >= g.S0 || sy >= g.SP) continue;
      const int c = g.f0 ? TILE - 1 - yl : yl;
      const T* p = from + sy * g.sp_stride + sx;
      if (sx + V <= g.S0) {
        const W w = vo_load<W>(p);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const int r = g.fa ? TILE - 1 - (xl + k) : xl + k;
          tile[((r / V) * GROUP + (r % V) * ROWD) * 4 / E + c] = vo_element<T, W>(w, k);
        }
      } else {
        for (int k = 0; k < V && sx + k < g.S0; ++k) {
          const int r = g.fa ? TILE - 1 - (xl + k) : xl + k;
          tile[((r / V) * GROUP + (r % V) * ROWD) * 4 / E + c] = p[k];
        }
      }
    }
    __syncthreads();
    const int i0_base = g.f0 ? g.SP - y0 - TILE : y0, ia_base = g.fa ? g.S0 - x0 - TILE : x0;      // (negative in a flipped edge tile)
    T* to = dst + (g.fb ? g.ST - 1 - st : st) * g.db_stride;
    for (int q = threadIdx.x; q < TILE * VO_LANES; q += VI_THREADS) {      // out: runs along destination x
      const int cw = q % VO_LANES, r = q / VO_LANES;
      const int i0 = i0_base + V * cw, ia = ia_base + r;
      if (ia < 0 || ia >= g.S0 || i0 + V <= 0 || i0 >= g.SP) continue;
      const int row = (r / V) * GROUP + (r % V) * ROWD;                    // dwords
      T* p = to + ia * g.da_stride;
      if (i0 >= 0 && i0 + V <= g.SP) {
        vo_store<W>(p + i0, lds[row * 4 / (int)sizeof(W) + cw]);
      } else {
        for (int k = 0; k < V; ++k)
          if (i0 + k >= 0 && i0 + k < g.SP) p[i0 + k] = tile[row * 4 / E + V * cw + k];
      }
    }
    __syncthreads();                           // the tile is free for the next piece of work
  }
}

template <typename T>
static void vo_launch(const void* src, int SX, int SY, int SZ, int p0, int p1, int p2, int flip_mask, void* dst, int64_t n, hipStream_t s) {
  typedef typename vo_word<T>::W W;
  constexpr int V = sizeof(W) / sizeof(T), TILE = VO_LANES * V;
  const int S[3] = {SX, SY, SZ}, P[3] = {p0, p1, p2};
  const int D[3] = {S[p0], S[p1], S[p2]};
  const int f[3] = {flip_mask & 1, (flip_mask >> 1) & 1, (flip_mask >> 2) & 1};
  if (p0 == 0) {
    const vo_rows g = {SX, D[1], SY, p1, f[0], f[1], f[2], D[2]};
    const int64_t words = mud_cdiv(n, V);
    hipLaunchKernelGGL(k_vo_rows<T>, dim3(vi_blocks(words, VI_THREADS, VO_MAX_BLOCKS)), dim3(VI_THREADS), 0, s, (const T*)src, (T*)dst, g, n, words);
    return;
  }
  const int a = P[1] == 0 ? 1 : 2, b = 3 - a, t = P[b];                    // destination axis a holds source x, b the source's third axis t
  const int64_t sstride[3] = {1, SX, (int64_t)SX * SY}, dstride[3] = {1, D[0], (int64_t)D[0] * D[1]};
  vo_tiles g;
  g.S0 = SX, g.SP = S[p0], g.ST = S[t];
  g.sp_stride = sstride[p0], g.st_stride = sstride[t];
  g.da_stride = dstride[a], g.db_stride = dstride[b];
  g.f0 = f[0], g.fa = f[a], g.fb = f[b];
  g.tiles_x = (int)mud_cdiv(g.S0, TILE), g.tiles_y = (int)mud_cdiv(g.SP, TILE);
  g.total = (int64_t)g.tiles_x * g.tiles_y * g.ST;
  hipLaunchKernelGGL(k_vo_tiles<T>, dim3(vi_blocks(g.total, 1, VO_MAX_BLOCKS)), dim3(VI_THREADS), 0, s, (const T*)src, (T*)dst, g);
}

extern "C" int mud_volume_reorient(const void* src, int elem_bytes, int SX, int SY, int SZ, int p0, int p1, int p2, int flip_mask, void* dst,
                                   void* stream) {
  MUD_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8, "mud_volume_reorient: elements of 1, 2, 4 or 8 bytes, got %d",
              elem_bytes);
  MUD_REQUIRE(p0 >= 0 && p0 <= 2 && p1 >= 0 && p1 <= 2 && p2 >= 0 && p2 <= 2 && p0 != p1 && p0 != p2 && p1 != p2,
              "mud_volume_reorient: (%d, %d, %d) is not a permutation of 0, 1, 2", p0, p1, p2);
  MUD_REQUIRE(flip_mask >= 0 && flip_mask <= 7, "mud_volume_reorient: flip mask %d is not in [0, 7]", flip_mask);
  MUD_REQUIRE(SX >= 0 && SY >= 0 && SZ >= 0, "mud_volume_reorient: bad volume size %d x %d x %d", SX, SY, SZ);
  const int64_t plane = (int64_t)SX * SY, lim = (int64_t)1 << 31;          // (each factor < 2^31: no product below overflows)
  if (plane == 0 || SZ == 0) return MUD_OK;                                // nothing to move
  MUD_REQUIRE(plane < lim && plane * SZ < lim, "mud_volume_reorient: bad volume size %d x %d x %d (2^31 voxels or more)", SX, SY, SZ);
  const int64_t n = plane * SZ;
  MUD_REQUIRE(src != nullptr && dst != nullptr, "mud_volume_reorient: null pointer");
  MUD_REQUIRE(vi_aligned(src, elem_bytes) && vi_aligned(dst, elem_bytes), "mud_volume_reorient: the volumes must be aligned to their %d-byte elements",
              elem_bytes);
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst, bytes = (uintptr_t)n * elem_bytes;
  MUD_REQUIRE(s0 + bytes <= d0 || d0 + bytes <= s0, "mud_volume_reorient: source and destination overlap (not an in-place operation)");
  hipStream_t s = (hipStream_t)stream;
  switch (elem_bytes) {
    case 1: vo_launch<uint8_t>(src, SX, SY, SZ, p0, p1, p2, flip_mask, dst, n, s); break;
    case 2: vo_launch<uint16_t>(src, SX, SY, SZ, p0, p1, p2, flip_mask, dst, n, s); break;
    case 4: vo_launch<uint32_t>(src, SX, SY, SZ, p0, p1, p2, flip_mask, dst, n, s); break;
    default: vo_launch<uint64_t>(src, SX, SY, SZ, p0, p1, p2, flip_mask, dst, n, s); break;
  }
  MUD_CHECK_LAUNCH("mud_volume_reorient");
  return MUD_OK;
}
