// Foreground masking of the volume pipeline's inputs (--foreground; include/mudiff_hip.h: mud_volume_fg_*; mudiff_hip.volume_foreground;
// DESIGN.md section 5.16): an Otsu threshold on a histogram of the candidates (the finite voxels that are != 0), an optional opening,
// the largest 6-connected component and its holes.  Everything here is integer work: every result is the same bits on every run and
// equals tests/volume_foreground_ref.py bit for bit.
//
// The labelling is a block-based union-find in three launches, none of which iterates "until nothing changes":
//   1  a workgroup labels its 32 x 8 x 4 tile in LDS: parent[l] = l for a member, every member is joined to its -x, -y and -z
//      neighbours inside the tile (fg_union with atomicMin on LDS), then every voxel writes the root of its tile-local tree as a global index
//   2  every member on the low x / y / z face of a tile is joined to its neighbour in the tile before it: the lock-free fg_union on
//      global memory, atomicMin on the larger root
//   3  every member replaces its parent by its root
// The invariant is parent[i] <= i at all times (volume_fg_unionfind.h): every find and every retry of a union strictly descends, so no
// loop can spin on another wave's progress.  Tile-local indices and global indices order the voxels of a tile alike (z, then y, then x),
// so the invariant carries over from pass 1 to pass 2.  The label of a component is its smallest linear index.
#include "volume_common.h"
#include "volume_fg_unionfind.h"

#define FG_TILE (VI_TX * VI_TY * VI_TZ)
#define FG_PER_THREAD (FG_TILE / VI_THREADS)   // a thread owns the voxels tid + k * VI_THREADS of the tile: (lx, ly) fixed, lz = k
#define FG_MIN_BINS 16
#define FG_MAX_BINS 1024
#define FG_FACE 0x80000000u                    // census[root]: the voxel count in the low 31 bits, this bit if the component touches a face

static_assert(FG_PER_THREAD == VI_TZ && VI_THREADS == VI_TX * VI_TY, "one thread per (x, y) column of the tile");

struct fg_lds_memory {                         // the tile's own parents: other waves of the workgroup merge into them meanwhile
  static __device__ __forceinline__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  static __device__ __forceinline__ int fetch_min(int* p, int v) { return atomicMin(p, v); }
};
struct fg_global_memory {                      // parents other workgroups merge into: loads that bypass this CU's L1
  static __device__ __forceinline__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ int fetch_min(int* p, int v) { return atomicMin(p, v); }
};

__device__ __forceinline__ bool fg_candidate(float v) { return vc_finite(v) && v != 0.0f; }

// ---- the range of the candidates: out[0] = max of ~key (so that 0 means "none"), out[1] = max of key, out[2] = their number
template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_fg_range(vi_source src, int64_t n, uint32_t* __restrict__ out) {
  __shared__ uint32_t s[3];
  if (threadIdx.x < 3) s[threadIdx.x] = 0;
  __syncthreads();
  uint32_t inv = 0, top = 0, cnt = 0;
  VI_GRID_STRIDE(i, n) {
    const float v = vi_at<T>(src, i);
    if (!fg_candidate(v)) continue;
    const uint32_t k = vc_key(v);
    inv = ~k > inv ? ~k : inv;
    top = k > top ? k : top;
    cnt += 1;
  }
  if (cnt) {
    atomicMax(&s[0], inv);
    atomicMax(&s[1], top);
    atomicAdd(&s[2], cnt);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s[2]) {
    atomicMax(&out[0], s[0]);
    atomicMax(&out[1], s[1]);
    atomicAdd(&out[2], s[2]);
  }
}

// ---- the histogram of the candidates
template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_fg_hist(vi_source src, int64_t n, double lo, double scale, int bins, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[FG_MAX_BINS];
  vc_hist_clear(h, bins);
  VI_GRID_STRIDE(i, n) {
    const float v = vi_at<T>(src, i);
    if (fg_candidate(v)) atomicAdd(&h[vc_bin(v, lo, scale, bins)], 1u);
  }
  vc_hist_merge(h, bins, hist);
}

// ---- the raw mask: a candidate whose bin is above k
template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_fg_mask(vi_source src, int64_t n, double lo, double scale, int bins, int k, uint8_t* __restrict__ mask) {
  VI_GRID_STRIDE(i, n) {
    const float v = vi_at<T>(src, i);
    mask[i] = (fg_candidate(v) && vc_bin(v, lo, scale, bins) > k) ? 1 : 0;
  }
}

// ---- one erosion (dilate == 0: on iff the voxel and its six neighbours are on, outside the volume counts as on) or one dilation (on iff
// any of the seven is on, outside counts as off); the tile and a halo of one voxel are staged in LDS
__global__ __launch_bounds__(VI_THREADS) void k_fg_morph(const uint8_t* __restrict__ in, int X, int Y, int Z, int dilate, uint8_t* __restrict__ out) {
  constexpr int SX = VI_TX + 2, SY = VI_TY + 2, SZ = VI_TZ + 2;
  __shared__ uint8_t s[SZ * SY * SX];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * VI_TX, y0 = blockIdx.y * VI_TY, z0 = blockIdx.z * VI_TZ;
  const uint8_t outside = dilate ? 0 : 1;
  for (int i = tid; i < SZ * SY * SX; i += VI_THREADS) {
    const int row = i / SX, ix = i - row * SX, iz = row / SY, iy = row - iz * SY;
    const int gx = x0 - 1 + ix, gy = y0 - 1 + iy, gz = z0 - 1 + iz;
    uint8_t v = outside;
    if (gx >= 0 && gx < X && gy >= 0 && gy < Y && gz >= 0 && gz < Z) v = in[((int64_t)gz * Y + gy) * X + gx] != 0;
    s[i] = v;
  }
  __syncthreads();
  const int lx = tid & (VI_TX - 1), ly = tid / VI_TX;
  const int gx = x0 + lx, gy = y0 + ly;
  if (gx >= X || gy >= Y) return;
#pragma unroll
  for (int lz = 0; lz < VI_TZ; ++lz) {
    const int gz = z0 + lz;
    if (gz >= Z) break;
    const int c = ((lz + 1) * SY + ly + 1) * SX + lx + 1;
    const int a = s[c], b = s[c - 1], d = s[c + 1], e = s[c - SX], f = s[c + SX], g = s[c - SX * SY], h = s[c + SX * SY];
    out[((int64_t)gz * Y + gy) * X + gx] = dilate ? (uint8_t)(a | b | d | e | f | g | h) : (uint8_t)(a & b & d & e & f & g & h);
  }
}

// ---- labelling, pass 1: the tile in LDS.  A member is a voxel whose mask equals `value`.
__global__ __launch_bounds__(VI_THREADS) void k_fg_label_tile(const uint8_t* __restrict__ mask, int X, int Y, int Z, int value, int* __restrict__ labels) {
  __shared__ int parent[FG_TILE];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * VI_TX, y0 = blockIdx.y * VI_TY, z0 = blockIdx.z * VI_TZ;
  const int lx = tid & (VI_TX - 1), ly = tid / VI_TX;
  const int gx = x0 + lx, gy = y0 + ly;
  const bool column = gx < X && gy < Y;
#pragma unroll
  for (int lz = 0; lz < VI_TZ; ++lz) {
    const int gz = z0 + lz, l = tid + lz * VI_THREADS;
    const bool member = column && gz < Z && (mask[((int64_t)gz * Y + gy) * X + gx] != 0) == (value != 0);
    parent[l] = member ? l : -1;
  }
  __syncthreads();
  // (whether a voxel is a member never changes: a -1 stays, an index stays an index; only which index may change under this thread)
#pragma unroll
  for (int lz = 0; lz < VI_TZ; ++lz) {
    const int l = tid + lz * VI_THREADS;
    if (parent[l] < 0) continue;
    if (lx > 0 && parent[l - 1] >= 0) fg_union<fg_lds_memory>(parent, l, l - 1);
    if (ly > 0 && parent[l - VI_TX] >= 0) fg_union<fg_lds_memory>(parent, l, l - VI_TX);
    if (lz > 0 && parent[l - VI_THREADS] >= 0) fg_union<fg_lds_memory>(parent, l, l - VI_THREADS);
  }
  __syncthreads();
  if (!column) return;
#pragma unroll
  for (int lz = 0; lz < VI_TZ; ++lz) {
    const int gz = z0 + lz, l = tid + lz * VI_THREADS;
    if (gz >= Z) break;
    int label = -1;
    if (parent[l] >= 0) {
      const int r = fg_find<fg_lds_memory>(parent, l);
      const int rx = r & (VI_TX - 1), ry = (r / VI_TX) & (VI_TY - 1), rz = r / VI_THREADS;
      label = (int)(((int64_t)(z0 + rz) * Y + (y0 + ry)) * X + (x0 + rx));       // < 2^31: the entry point checks the size
    }
    labels[((int64_t)gz * Y + gy) * X + gx] = label;
  }
}

// ---- labelling, pass 2: the faces between tiles
__global__ __launch_bounds__(VI_THREADS) void k_fg_label_merge(const uint8_t* __restrict__ mask, int X, int Y, int Z, int value, int64_t n, int* labels) {
  const bool on = value != 0;
  VI_GRID_STRIDE(i, n) {
    int x, y, z;
    vi_xyz(i, X, Y, x, y, z);
    const bool fx = x > 0 && (x & (VI_TX - 1)) == 0, fy = y > 0 && (y & (VI_TY - 1)) == 0, fz = z > 0 && (z & (VI_TZ - 1)) == 0;
    if (!(fx || fy || fz)) continue;
    if ((mask[i] != 0) != on) continue;
    const int64_t sy = X, sz = (int64_t)X * Y;
    if (fx && (mask[i - 1] != 0) == on) fg_union<fg_global_memory>(labels, (int)i, (int)(i - 1));
    if (fy && (mask[i - sy] != 0) == on) fg_union<fg_global_memory>(labels, (int)i, (int)(i - sy));
    if (fz && (mask[i - sz] != 0) == on) fg_union<fg_global_memory>(labels, (int)i, (int)(i - sz));
  }
}

// ---- labelling, pass 3: every member takes its root.  A parent another thread has replaced by the root meanwhile is as good as the older one.
__global__ __launch_bounds__(VI_THREADS) void k_fg_label_flatten(int64_t n, int* labels) {
  VI_GRID_STRIDE(i, n) {
    const int p = fg_global_memory::load(labels + i);
    if (p < 0 || p == (int)i) continue;
    __hip_atomic_store(labels + i, fg_find<fg_global_memory>(labels, p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- the census of the components: census[root] = the number of voxels, and FG_FACE if one of them lies on a face of the volume.  The
// lanes of a wave that hold the same root add once: the loop below retires at least its leader per round, 64 rounds at the most.
__global__ __launch_bounds__(VI_THREADS) void k_fg_census(const int* __restrict__ labels, int X, int Y, int Z, int64_t n, uint32_t* __restrict__ census) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * VI_THREADS; base < n; base += (int64_t)gridDim.x * VI_THREADS) {
    const int64_t i = base + threadIdx.x;
    int r = -1;
    bool face = false;
    if (i < n) {
      r = labels[i];
      int x, y, z;
      vi_xyz(i, X, Y, x, y, z);
      face = x == 0 || x == X - 1 || y == 0 || y == Y - 1 || z == 0 || z == Z - 1;
    }
    bool todo = r >= 0;
    for (;;) {
      const unsigned long long open = __ballot(todo);
      if (!open) break;
      const int leader = __ffsll(open) - 1;
      const int root = __shfl(r, leader, 64);
      const bool same = todo && r == root;
      const unsigned long long group = __ballot(same), onface = __ballot(same && face);
      if (lane == leader) {
        atomicAdd(&census[root], (uint32_t)__popcll(group));
        if (onface) atomicOr(&census[root], FG_FACE);
      }
      if (same) todo = false;
    }
  }
}

// ---- the winner: summary[0] = max over the roots of (count << 32) | (0xFFFFFFFF - root), summary[1] = the number of roots
__global__ __launch_bounds__(VI_THREADS) void k_fg_winner(const int* __restrict__ labels, const uint32_t* __restrict__ census, int64_t n,
                                                          unsigned long long* __restrict__ summary) {
  __shared__ unsigned long long s[2];
  if (threadIdx.x < 2) s[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long best = 0, roots = 0;
  VI_GRID_STRIDE(i, n) {
    if (labels[i] != (int)i) continue;
    const unsigned long long packed = ((unsigned long long)(census[i] & ~FG_FACE) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
    best = packed > best ? packed : best;
    roots += 1;
  }
  if (roots) {
    atomicMax(&s[0], best);
    atomicAdd(&s[1], roots);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s[1]) {
    atomicMax(&summary[0], s[0]);
    atomicAdd(&summary[1], s[1]);
  }
}

// ---- holes == 0: mask = (label == root).  holes != 0: every labelled voxel whose component does not touch a face is switched on.
// count: the voxels switched on
__global__ __launch_bounds__(VI_THREADS) void k_fg_select(const int* __restrict__ labels, const uint32_t* __restrict__ census, int root, int holes,
                                                          int64_t n, uint8_t* __restrict__ mask, uint32_t* __restrict__ count) {
  __shared__ uint32_t s;                       // the workgroup's count: a histogram of one bin
  vc_hist_clear(&s, 1);
  uint32_t mine = 0;
  VI_GRID_STRIDE(i, n) {
    const int r = labels[i];
    if (holes) {
      if (r >= 0 && !(census[r] & FG_FACE)) {
        mask[i] = 1;
        mine += 1;
      }
    } else {
      const bool keep = r == root;
      mask[i] = keep ? 1 : 0;
      mine += keep ? 1 : 0;
    }
  }
  if (mine) atomicAdd(&s, mine);
  vc_hist_merge(&s, 1, count);
}

// ---- the output: the voxel's value inside the mask (whatever its bits), +0 outside; removed: the candidates outside
template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_fg_apply(vi_source src, int64_t n, const uint8_t* __restrict__ mask, float* __restrict__ out,
                                                         uint32_t* __restrict__ removed) {
  __shared__ uint32_t s;                       // the workgroup's count: a histogram of one bin
  vc_hist_clear(&s, 1);
  uint32_t mine = 0;
  VI_GRID_STRIDE(i, n) {
    const float v = vi_at<T>(src, i);
    const bool in = mask[i] != 0;
    if (!in && fg_candidate(v)) mine += 1;
    out[i] = in ? v : 0.0f;
  }
  if (mine) atomicAdd(&s, mine);
  vc_hist_merge(&s, 1, removed);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------
static inline int fg_check_grid(const char* who, int X, int Y, int Z) {
  if (int e = vi_check_size(who, "volume", X, Y, Z)) return e;
  return vi_check_tiled(who, X, Y, Z);
}

static inline int fg_check_bins(const char* who, double lo, double scale, int bins) {
  if (int e = vi_check_bins(who, lo, scale, bins, FG_MIN_BINS, FG_MAX_BINS)) return e;
  MUD_REQUIRE(scale > 0.0, "%s: scale must be positive (got %g)", who, scale);
  return MUD_OK;
}

extern "C" int mud_volume_fg_range(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, uint32_t* range, void* stream) {
  if (int e = vi_check_volume("mud_volume_fg_range", vol, datatype, X, Y, Z)) return e;
  MUD_REQUIRE(range != nullptr && vi_aligned(range, 4), "mud_volume_fg_range: range must be a 4-byte aligned pointer");
  hipStream_t s = (hipStream_t)stream;
  if (int e = vi_clear("mud_volume_fg_range", range, 3 * sizeof(uint32_t), s)) return e;
  const int64_t n = (int64_t)X * Y * Z;
  VI_DISPATCH(datatype, hipLaunchKernelGGL(k_fg_range<T>, dim3(vi_blocks(n)), dim3(VI_THREADS), 0, s, vi_source_of(vol, datatype, slope, inter), n,
                                           range));
  MUD_CHECK_LAUNCH("mud_volume_fg_range");
  return MUD_OK;
}

extern "C" int mud_volume_fg_hist(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, double lo, double scale, int bins,
                                  uint32_t* hist, void* stream) {
  if (int e = vi_check_volume("mud_volume_fg_hist", vol, datatype, X, Y, Z)) return e;
  if (int e = fg_check_bins("mud_volume_fg_hist", lo, scale, bins)) return e;
  MUD_REQUIRE(hist != nullptr && vi_aligned(hist, 4), "mud_volume_fg_hist: hist must be a 4-byte aligned pointer");
  hipStream_t s = (hipStream_t)stream;
  if (int e = vi_clear("mud_volume_fg_hist", hist, sizeof(uint32_t) * bins, s)) return e;
  const int64_t n = (int64_t)X * Y * Z;
  VI_DISPATCH(datatype, hipLaunchKernelGGL(k_fg_hist<T>, dim3(vi_blocks(n)), dim3(VI_THREADS), 0, s, vi_source_of(vol, datatype, slope, inter), n,
                                           lo, scale, bins, hist));
  MUD_CHECK_LAUNCH("mud_volume_fg_hist");
  return MUD_OK;
}

extern "C" int mud_volume_fg_mask(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, double lo, double scale, int bins,
                                  int k, uint8_t* mask, void* stream) {
  if (int e = vi_check_volume("mud_volume_fg_mask", vol, datatype, X, Y, Z)) return e;
  if (int e = fg_check_bins("mud_volume_fg_mask", lo, scale, bins)) return e;
  MUD_REQUIRE(k >= 0 && k <= bins - 2, "mud_volume_fg_mask: the threshold bin %d is not in [0, %d]", k, bins - 2);
  MUD_REQUIRE(mask != nullptr && (const void*)mask != vol, "mud_volume_fg_mask: mask must be a buffer of its own");
  const int64_t n = (int64_t)X * Y * Z;
  VI_DISPATCH(datatype, hipLaunchKernelGGL(k_fg_mask<T>, dim3(vi_blocks(n)), dim3(VI_THREADS), 0, (hipStream_t)stream,
                                           vi_source_of(vol, datatype, slope, inter), n, lo, scale, bins, k, mask));
  MUD_CHECK_LAUNCH("mud_volume_fg_mask");
  return MUD_OK;
}

extern "C" int mud_volume_fg_morph(const uint8_t* in, int X, int Y, int Z, int dilate, uint8_t* out, void* stream) {
  if (int e = fg_check_grid("mud_volume_fg_morph", X, Y, Z)) return e;
  MUD_REQUIRE(in != nullptr && out != nullptr, "mud_volume_fg_morph: null pointer");
  MUD_REQUIRE(in != out, "mud_volume_fg_morph: out must be a buffer of its own");
  MUD_REQUIRE(dilate == 0 || dilate == 1, "mud_volume_fg_morph: dilate must be 0 (erode) or 1 (got %d)", dilate);
  hipLaunchKernelGGL(k_fg_morph, vi_tile_grid(X, Y, Z), dim3(VI_THREADS), 0, (hipStream_t)stream, in, X, Y, Z, dilate, out);
  MUD_CHECK_LAUNCH("mud_volume_fg_morph");
  return MUD_OK;
}

extern "C" int mud_volume_fg_label(const uint8_t* mask, int X, int Y, int Z, int value, int32_t* labels, void* stream) {
  if (int e = fg_check_grid("mud_volume_fg_label", X, Y, Z)) return e;
  MUD_REQUIRE(mask != nullptr && labels != nullptr, "mud_volume_fg_label: null pointer");
  MUD_REQUIRE(vi_aligned(labels, 4), "mud_volume_fg_label: labels must be 4-byte aligned");
  MUD_REQUIRE(value == 0 || value == 1, "mud_volume_fg_label: the value to label must be 0 or 1 (got %d)", value);
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)X * Y * Z;
  hipLaunchKernelGGL(k_fg_label_tile, vi_tile_grid(X, Y, Z), dim3(VI_THREADS), 0, s, mask, X, Y, Z, value, labels);
  hipLaunchKernelGGL(k_fg_label_merge, dim3(vi_blocks(n)), dim3(VI_THREADS), 0, s, mask, X, Y, Z, value, n, labels);
  hipLaunchKernelGGL(k_fg_label_flatten, dim3(vi_blocks(n)), dim3(VI_THREADS), 0, s, n, labels);
  MUD_CHECK_LAUNCH("mud_volume_fg_label");
  return MUD_OK;
}

extern "C" int mud_volume_fg_census(const int32_t* labels, int X, int Y, int Z, uint32_t* census, uint64_t* summary, void* stream) {
  if (int e = fg_check_grid("mud_volume_fg_census", X, Y, Z)) return e;
  MUD_REQUIRE(labels != nullptr && census != nullptr && summary != nullptr, "mud_volume_fg_census: null pointer");
  MUD_REQUIRE(vi_aligned(labels, 4) && vi_aligned(census, 4) && vi_aligned(summary, 8),
              "mud_volume_fg_census: labels and census must be 4-byte aligned, summary 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)X * Y * Z;
  if (int e = vi_clear("mud_volume_fg_census", census, sizeof(uint32_t) * (size_t)n, s)) return e;
  if (int e = vi_clear("mud_volume_fg_census", summary, 2 * sizeof(uint64_t), s)) return e;
  hipLaunchKernelGGL(k_fg_census, dim3(vi_blocks(n)), dim3(VI_THREADS), 0, s, labels, X, Y, Z, n, census);
  hipLaunchKernelGGL(k_fg_winner, dim3(vi_blocks(n)), dim3(VI_THREADS), 0, s, labels, census, n, (unsigned long long*)summary);
  MUD_CHECK_LAUNCH("mud_volume_fg_census");
  return MUD_OK;
}

extern "C" int mud_volume_fg_select(const int32_t* labels, const uint32_t* census, int64_t n, int root, int holes, uint8_t* mask, uint32_t* count,
                                    void* stream) {
  MUD_REQUIRE(n > 0 && n < ((int64_t)1 << 31), "mud_volume_fg_select: bad voxel count %lld", (long long)n);
  MUD_REQUIRE(labels != nullptr && mask != nullptr && count != nullptr, "mud_volume_fg_select: null pointer");
  MUD_REQUIRE(vi_aligned(labels, 4) && vi_aligned(count, 4), "mud_volume_fg_select: labels and count must be 4-byte aligned");
  MUD_REQUIRE(holes == 0 || holes == 1, "mud_volume_fg_select: holes must be 0 or 1 (got %d)", holes);
  if (holes)
    MUD_REQUIRE(census != nullptr && vi_aligned(census, 4), "mud_volume_fg_select: filling the holes needs the census");
  else
    MUD_REQUIRE(root >= 0 && root < n, "mud_volume_fg_select: the root %d is not a voxel of the volume", root);
  hipStream_t s = (hipStream_t)stream;
  if (int e = vi_clear("mud_volume_fg_select", count, sizeof(uint32_t), s)) return e;
  hipLaunchKernelGGL(k_fg_select, dim3(vi_blocks(n)), dim3(VI_THREADS), 0, s, labels, census, root, holes, n, mask, count);
  MUD_CHECK_LAUNCH("mud_volume_fg_select");
  return MUD_OK;
}

extern "C" int mud_volume_fg_apply(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, const uint8_t* mask, float* out,
                                   uint32_t* removed, void* stream) {
  if (int e = vi_check_volume("mud_volume_fg_apply", vol, datatype, X, Y, Z)) return e;
  MUD_REQUIRE(mask != nullptr && out != nullptr && removed != nullptr, "mud_volume_fg_apply: null pointer");
  MUD_REQUIRE((const void*)out != vol, "mud_volume_fg_apply: out must be a buffer of its own");
  MUD_REQUIRE(vi_aligned(out, 4) && vi_aligned(removed, 4), "mud_volume_fg_apply: out and removed must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (int e = vi_clear("mud_volume_fg_apply", removed, sizeof(uint32_t), s)) return e;
  const int64_t n = (int64_t)X * Y * Z;
  VI_DISPATCH(datatype, hipLaunchKernelGGL(k_fg_apply<T>, dim3(vi_blocks(n)), dim3(VI_THREADS), 0, s, vi_source_of(vol, datatype, slope, inter), n,
                                           mask, out, removed));
  MUD_CHECK_LAUNCH("mud_volume_fg_apply");
  return MUD_OK;
}
