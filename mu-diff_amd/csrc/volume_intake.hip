// On-device NIfTI intake and re-assembly of the volume pipeline (include/mudiff_hip.h: mud_volume_census, mud_volume_slab_normalise,
// mud_volume_slab_zscore, mud_volume_assemble, mud_volume_regrid; mudiff_hip.volume_intake, mudiff_hip.volume_regrid).
//
// A volume arrives exactly as the file stores it: x fastest ([Z][Y][X] in C terms), in the file's datatype, with scl_slope / scl_inter
// still to be applied.  Three things happen to it on the device:
//  - census: the order statistics volume.robust_minmax_to_minus1_1 needs (count, min, max and a 16-wide window of exact sorted values
//    around each requested percentile rank) by a radix select on the order-preserving uint32 image of the fp32 value.  8-bit digits,
//    four histogram passes (LDS-privatised, one read of the volume per pass serving every target rank), then one gathering pass for
//    the few keys strictly between a window's end keys.  Counts are integers: the result does not depend on the order of the atomics.
//  - slab normalise: clip((v - lo) / den, 0, 1) * 2 - 1 of the planes s0..s1 in fp32, each step rounded once, written as [n][X][Y]
//    (the transposed plane the sampler takes) through an LDS tile so that reads and writes are both coalesced; slab z-score
//    (--norm zscore) is the same tile with clamp((v - mean) / std, -3, 3) / 3, the moments coming from the host;
//  - assemble: the inverse transpose of predicted [n][X][Y] planes into a zero-filled volume in file order.
// In front of all that, mud_volume_regrid (--regrid) resamples a volume that lies on another voxel grid onto
// the grid of the first input: a gather through the affines, trilinear or nearest.
// DESIGN.md section 5.10 has the definitions and why they equal the host's results bit for bit.
#include "volume_common.h"

typedef uint32_t vi_u32x4 __attribute__((ext_vector_type(4)));

#define VI_TILE 64
#define VI_NT (2 + 2 * MUD_VI_MAX_RANKS)      // select targets: min, max, and the two ends of every window
#define VI_BETWEEN 16                         // capacity per window of the keys strictly between its end keys (at most 14 exist)

// device state of one census (the head of the workspace); zeroed by the entry point
struct vi_state {
  uint32_t hist[4][VI_NT][256];             // [pass][group leader][digit]
  uint32_t prefix[VI_NT];                   // the target's key so far (digits of the passes done, high bits)
  uint32_t below[VI_NT];                    // selected keys strictly below the target's prefix range
  uint32_t rank[VI_NT];                     // the target's rank in [0, n)
  uint32_t eq[VI_NT];                       // after the last pass: selected keys equal to the target's key
  int32_t leader[VI_NT];                    // first target with the same prefix (it owns the histogram row); -1: inactive
  uint32_t n, nonfinite;
  uint32_t nbetween[MUD_VI_MAX_RANKS];
  uint32_t between[MUD_VI_MAX_RANKS][VI_BETWEEN];
};

// f(value) for every voxel: 16-byte loads (the base is 16-byte aligned), the tail by the first threads of block 0
template <typename T, typename F>
__device__ __forceinline__ void vi_foreach(const vi_source& src, int64_t n, F f) {
  constexpr int V = 16 / (int)sizeof(T);
  const int64_t nvec = n / V;
  const vi_u32x4* __restrict__ pv = reinterpret_cast<const vi_u32x4*>(src.vol);
  VI_GRID_STRIDE(i, nvec) {
    union {
      vi_u32x4 w;
      T e[V];
    } u;
    u.w = pv[i];
#pragma unroll
    for (int j = 0; j < V; ++j) f(vi_value<T>(u.e[j], src.scaled, src.slope, src.inter));
  }
  if (blockIdx.x == 0) {
    const int64_t i = nvec * V + threadIdx.x;
    if (threadIdx.x < V && i < n) f(vi_at<T>(src, i));
  }
}

// one histogram pass: pass 0 counts the top digit of every selected key (and the non-finite ones); pass p > 0 counts digit p of the
// keys that share a target's prefix, once per group of targets with the same prefix
template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_vi_hist(vi_source src, int64_t n, int pass, vi_state* __restrict__ st) {
  __shared__ uint32_t h[VI_NT][256];
  __shared__ uint32_t s_prefix[VI_NT];
  __shared__ int s_lead[VI_NT];
  __shared__ uint32_t s_nonfinite;
  if (pass > 0 && st->n == 0) return;
  for (int i = threadIdx.x; i < VI_NT * 256; i += VI_THREADS) (&h[0][0])[i] = 0;
  if (threadIdx.x < VI_NT) {
    s_prefix[threadIdx.x] = st->prefix[threadIdx.x];
    s_lead[threadIdx.x] = pass == 0 ? (threadIdx.x == 0 ? 0 : -1) : st->leader[threadIdx.x];
  }
  if (threadIdx.x == 0) s_nonfinite = 0;
  __syncthreads();
  const int hi_shift = 32 - 8 * pass, lo_shift = 24 - 8 * pass;
  vi_foreach<T>(src, n, [&](float v) {
    if (!(v != 0.0f)) return;                 // selection: value != 0 (a NaN is selected, like numpy's data != 0)
    const uint32_t k = vi_key(v);
    if (pass == 0) {
      atomicAdd(&h[0][k >> 24], 1u);
      if (!vc_finite(v)) atomicAdd(&s_nonfinite, 1u);
    } else {
#pragma unroll
      for (int t = 0; t < VI_NT; ++t)
        if (s_lead[t] == t && ((k ^ s_prefix[t]) >> hi_shift) == 0) atomicAdd(&h[t][(k >> lo_shift) & 255u], 1u);
    }
  });
  __syncthreads();
  for (int i = threadIdx.x; i < VI_NT * 256; i += VI_THREADS) {
    const int t = i >> 8;
    const uint32_t c = h[t][i & 255];
    if (c && s_lead[t] == t) atomicAdd(&st->hist[pass][t][i & 255], c);
  }
  if (pass == 0 && threadIdx.x == 0 && s_nonfinite) atomicAdd(&st->nonfinite, s_nonfinite);
}

// after pass `pass`: every target descends into the digit that holds its rank.  One block; thread t < VI_NT owns target t.
__global__ __launch_bounds__(64) void k_vi_scan(vi_state* __restrict__ st, int pass, int nq, double q0, double q1, double q2, double q3) {
  const int t = threadIdx.x;
  __shared__ uint32_t s_prefix[VI_NT];
  __shared__ int s_active[VI_NT];
  if (pass == 0) {
    __shared__ uint32_t s_n;
    if (t == 0) {
      uint32_t n = 0;
      for (int b = 0; b < 256; ++b) n += st->hist[0][0][b];
      s_n = n;
      st->n = n;
    }
    __syncthreads();
    if (t < VI_NT) {
      const uint32_t n = s_n;
      int active = n > 0 && (t < 2 || (t - 2) / 2 < nq);
      uint32_t r = 0;
      if (active) {
        if (t == 0) r = 0;
        else if (t == 1) r = n - 1;
        else {
          const int i = (t - 2) / 2;
          const double q = i == 0 ? q0 : i == 1 ? q1 : i == 2 ? q2 : q3;
          const int64_t c = (int64_t)floor((double)(n - 1) * q);         // the window is centred on floor((n-1) q), in fp64
          const int64_t a = c - 8 < 0 ? 0 : c - 8, b = c + 7 > (int64_t)n - 1 ? (int64_t)n - 1 : c + 7;
          r = (uint32_t)(((t - 2) & 1) ? b : a);
        }
      }
      st->rank[t] = r;
      st->below[t] = 0;
      st->prefix[t] = 0;
      st->leader[t] = active ? 0 : -1;       // pass 0 has one histogram row, owned by target 0
    }
    __syncthreads();
  }
  if (st->n == 0) return;
  const int shift = 24 - 8 * pass;
  int active = 0;
  if (t < VI_NT) {
    const int lead = st->leader[t];
    active = lead >= 0;
    if (active) {
      const uint32_t want = st->rank[t] - st->below[t];     // rank inside the prefix range
      uint32_t cum = 0, cnt = 0;
      int b = 0;
      for (; b < 256; ++b) {
        cnt = st->hist[pass][lead][b];
        if (want < cum + cnt) break;
        cum += cnt;
      }
      if (b == 256) {                        // cannot happen for a consistent histogram; keep the indices in range regardless
        b = 255;
        cum -= cnt;
      }
      st->below[t] += cum;
      st->prefix[t] |= (uint32_t)b << shift;
      if (pass == 3) st->eq[t] = cnt;
    }
    s_prefix[t] = st->prefix[t];
    s_active[t] = active;
  }
  __syncthreads();
  if (t < VI_NT) {                           // regroup: the first active target with the same prefix owns the next pass's row
    int lead = -1;
    if (active)
      for (int u = 0; u <= t; ++u)
        if (s_active[u] && s_prefix[u] == s_prefix[t]) {
          lead = u;
          break;
        }
    st->leader[t] = lead;
  }
}

// the keys strictly between the end keys of each window (at most 14 per window, by the ranks of the ends)
template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_vi_gather(vi_source src, int64_t n, int nq, vi_state* __restrict__ st) {
  __shared__ uint32_t s_lo[MUD_VI_MAX_RANKS], s_hi[MUD_VI_MAX_RANKS];
  if (st->n == 0) return;
  if (threadIdx.x < MUD_VI_MAX_RANKS) {
    s_lo[threadIdx.x] = st->prefix[2 + 2 * threadIdx.x];
    s_hi[threadIdx.x] = st->prefix[3 + 2 * threadIdx.x];
  }
  __syncthreads();
  vi_foreach<T>(src, n, [&](float v) {
    if (!(v != 0.0f)) return;
    const uint32_t k = vi_key(v);
    for (int i = 0; i < nq; ++i)
      if (k > s_lo[i] && k < s_hi[i]) {
        const uint32_t slot = atomicAdd(&st->nbetween[i], 1u);
        if (slot < VI_BETWEEN) st->between[i][slot] = k;
      }
  });
}

// the record: thread i < nq writes window i
__global__ __launch_bounds__(64) void k_vi_finish(vi_state* __restrict__ st, int nq, mud_volume_census_record* __restrict__ rec) {
  const int i = threadIdx.x;
  const uint32_t n = st->n;
  if (i == 0) {
    rec->n = n;
    rec->n_nonfinite = st->nonfinite;
    rec->min = n ? vi_unkey(st->prefix[0]) : 0.0f;
    rec->max = n ? vi_unkey(st->prefix[1]) : 0.0f;
  }
  if (i >= MUD_VI_MAX_RANKS) return;
  int64_t first = 0;
  int count = 0;
  float w[MUD_VI_WINDOW];
  for (int j = 0; j < MUD_VI_WINDOW; ++j) w[j] = 0.0f;
  if (i < nq && n > 0) {
    const int ta = 2 + 2 * i, tb = 3 + 2 * i;
    const uint32_t a = st->rank[ta], b = st->rank[tb];
    const uint32_t ka = st->prefix[ta], kb = st->prefix[tb];
    const uint32_t end_a = st->below[ta] + st->eq[ta];      // ranks [below_a, end_a) hold ka, [below_b, ...) hold kb
    const uint32_t below_b = st->below[tb];
    uint32_t nb = st->nbetween[i] < VI_BETWEEN ? st->nbetween[i] : VI_BETWEEN;
    uint32_t s[VI_BETWEEN];
    for (uint32_t j = 0; j < nb; ++j) s[j] = st->between[i][j];
    for (uint32_t j = 1; j < nb; ++j) {                      // insertion sort of at most 14 keys
      const uint32_t k = s[j];
      int m = (int)j - 1;
      while (m >= 0 && s[m] > k) {
        s[m + 1] = s[m];
        --m;
      }
      s[m + 1] = k;
    }
    first = a;
    count = (int)(b - a + 1);
    for (int j = 0; j < count && j < MUD_VI_WINDOW; ++j) {
      const uint32_t r = a + (uint32_t)j;
      uint32_t k;
      if (r < end_a) k = ka;
      else if (r >= below_b) k = kb;
      else {
        const uint32_t m = r - end_a;
        k = m < nb ? s[m] : kb;
      }
      w[j] = vi_unkey(k);
    }
  }
  rec->first_rank[i] = first;
  rec->count[i] = count;
  for (int j = 0; j < MUD_VI_WINDOW; ++j) rec->window[i][j] = w[j];
}

extern "C" int64_t mud_volume_census_ws_bytes(void) { return (int64_t)((sizeof(vi_state) + 255) / 256 * 256); }

extern "C" int mud_volume_census(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, const double* q, int nq,
                                 mud_volume_census_record* record, void* ws, int64_t ws_bytes, void* stream) {
  if (int e = vi_check_volume("mud_volume_census", vol, datatype, X, Y, Z)) return e;
  MUD_REQUIRE(nq >= 0 && nq <= MUD_VI_MAX_RANKS, "mud_volume_census: 0 to %d ranks, got %d", MUD_VI_MAX_RANKS, nq);
  MUD_REQUIRE(nq == 0 || q != nullptr, "mud_volume_census: null pointer (q)");
  double qq[MUD_VI_MAX_RANKS] = {0, 0, 0, 0};
  for (int i = 0; i < nq; ++i) {
    MUD_REQUIRE(q[i] >= 0.0 && q[i] <= 1.0, "mud_volume_census: q[%d] = %g is not a fraction in [0, 1]", i, q[i]);
    qq[i] = q[i];
  }
  MUD_REQUIRE(record != nullptr && ws != nullptr, "mud_volume_census: null pointer");
  MUD_REQUIRE(vi_aligned(record, 8) && vi_aligned(ws, 8), "mud_volume_census: record and ws must be 8-byte aligned");
  MUD_REQUIRE(ws_bytes >= mud_volume_census_ws_bytes(), "mud_volume_census: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
              (long long)mud_volume_census_ws_bytes());
  hipStream_t s = (hipStream_t)stream;
  vi_state* st = (vi_state*)ws;
  const int64_t n = (int64_t)X * Y * Z;
  const vi_source src = vi_source_of(vol, datatype, slope, inter);
  const unsigned blocks = vi_blocks(mud_cdiv(n, 16 / vi_esize(datatype)), VI_THREADS, VI_MAX_BLOCKS);      // a thread reads 16 bytes at a time
  if (int e = vi_clear("mud_volume_census", st, sizeof(vi_state), s)) return e;
  for (int pass = 0; pass < 4; ++pass) {
    VI_DISPATCH(datatype, hipLaunchKernelGGL(k_vi_hist<T>, dim3(blocks), dim3(VI_THREADS), 0, s, src, n, pass, st));
    MUD_CHECK_LAUNCH("mud_volume_census (histogram)");
    hipLaunchKernelGGL(k_vi_scan, dim3(1), dim3(64), 0, s, st, pass, nq, qq[0], qq[1], qq[2], qq[3]);
    MUD_CHECK_LAUNCH("mud_volume_census (scan)");
  }
  if (nq > 0) {
    VI_DISPATCH(datatype, hipLaunchKernelGGL(k_vi_gather<T>, dim3(blocks), dim3(VI_THREADS), 0, s, src, n, nq, st));
    MUD_CHECK_LAUNCH("mud_volume_census (gather)");
  }
  hipLaunchKernelGGL(k_vi_finish, dim3(1), dim3(64), 0, s, st, nq, record);
  MUD_CHECK_LAUNCH("mud_volume_census (record)");
  return MUD_OK;
}

// ---- slab normalise: stored planes [Y][X] of z = s0..s1 -> out [n][X][Y] ---------------------------------------------------------------
__device__ __forceinline__ float vi_normalise(float v, float lo, float den) {
#pragma clang fp contract(off)
  float t = v - lo;
  t = t / den;                                 // correctly rounded fp32 division
  t = t != t ? t : fminf(fmaxf(t, 0.0f), 1.0f);  // np.clip keeps a NaN
  t = t * 2.0f;
  return t - 1.0f;
}

// the tile both slab kernels share: f(value) of the 64 x 64 voxels at (x0, y0) of stored plane s0 + i goes through LDS, so that the
// reads run along x and the writes of out[i][x][y] along y (row stride 65 words: a column read touches 64 different banks)
template <typename T, typename F>
__device__ __forceinline__ void vi_slab_tile(const vi_source& src, int X, int Y, int s0, float* __restrict__ out, F f) {
  __shared__ float tile[VI_TILE][VI_TILE + 1];
  const int x0 = blockIdx.x * VI_TILE, y0 = blockIdx.y * VI_TILE, i = blockIdx.z;
  const int lx = threadIdx.x & (VI_TILE - 1), r0 = threadIdx.x / VI_TILE;
  const int64_t plane = (int64_t)(s0 + i) * X * Y;
  for (int r = r0; r < VI_TILE; r += VI_THREADS / VI_TILE) {                 // row r of the tile: y = y0 + r, lanes along x
    const int x = x0 + lx, y = y0 + r;
    if (x < X && y < Y) tile[r][lx] = f(vi_at<T>(src, plane + (int64_t)y * X + x));
  }
  __syncthreads();
  float* __restrict__ dst = out + (int64_t)i * X * Y;
  for (int r = r0; r < VI_TILE; r += VI_THREADS / VI_TILE) {                 // row r of the output tile: x = x0 + r, lanes along y
    const int x = x0 + r, y = y0 + lx;
    if (x < X && y < Y) dst[(int64_t)x * Y + y] = tile[lx][r];
  }
}

template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_vi_slab(vi_source src, int X, int Y, int s0, float lo, float den, int degenerate,
                                                        float* __restrict__ out) {
  vi_slab_tile<T>(src, X, Y, s0, out, [=](float v) { return degenerate ? 0.0f : vi_normalise(v, lo, den); });
}

extern "C" int mud_volume_slab_normalise(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, float lo, float den,
                                         int degenerate, int s0, int s1, float* out, void* stream) {
  if (int e = vi_check_volume("mud_volume_slab_normalise", vol, datatype, X, Y, Z)) return e;
  MUD_REQUIRE(s0 >= 0 && s1 >= s0 && s1 < Z, "mud_volume_slab_normalise: the slab %d..%d is not inside the %d planes", s0, s1, Z);
  MUD_REQUIRE(out != nullptr, "mud_volume_slab_normalise: null pointer");
  MUD_REQUIRE(degenerate || (den == den && lo == lo), "mud_volume_slab_normalise: lo / den must not be NaN");
  const dim3 grid((unsigned)mud_cdiv(X, VI_TILE), (unsigned)mud_cdiv(Y, VI_TILE), (unsigned)(s1 - s0 + 1));
  MUD_REQUIRE(grid.y <= 65535 && grid.z <= 65535, "mud_volume_slab_normalise: the volume is too large");
  VI_DISPATCH(datatype, hipLaunchKernelGGL(k_vi_slab<T>, grid, dim3(VI_THREADS), 0, (hipStream_t)stream, vi_source_of(vol, datatype, slope, inter),
                                           X, Y, s0, lo, den, degenerate, out));
  MUD_CHECK_LAUNCH("mud_volume_slab_normalise");
  return MUD_OK;
}

// ---- slab z-score: the training normalisation, clamp((v - mean) / std, -3, 3) / 3 ------------------------------------------------------
__device__ __forceinline__ float vi_zscore(float v, float mean, float std) {
#pragma clang fp contract(off)
  float t = v - mean;
  t = t / std;                                     // correctly rounded fp32 division
  t = t != t ? t : fminf(fmaxf(t, -3.0f), 3.0f);   // torch.clamp keeps a NaN
  return t / 3.0f;                                 // a division, like torch on the CPU: x * (1 / 3) rounds differently
}

template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_vi_slab_zscore(vi_source src, int X, int Y, int s0, float mean, float std,
                                                               float* __restrict__ out) {
  vi_slab_tile<T>(src, X, Y, s0, out, [=](float v) { return vi_zscore(v, mean, std); });
}

extern "C" int mud_volume_slab_zscore(const void* vol, int datatype, int X, int Y, int Z, float slope, float inter, float mean, float std,
                                      int s0, int s1, float* out, void* stream) {
  if (int e = vi_check_volume("mud_volume_slab_zscore", vol, datatype, X, Y, Z)) return e;
  MUD_REQUIRE(s0 >= 0 && s1 >= s0 && s1 < Z, "mud_volume_slab_zscore: the slab %d..%d is not inside the %d planes", s0, s1, Z);
  MUD_REQUIRE(out != nullptr, "mud_volume_slab_zscore: null pointer");
  MUD_REQUIRE(std != 0.0f, "mud_volume_slab_zscore: std must not be 0 (a flat volume passes 1)");
  const dim3 grid((unsigned)mud_cdiv(X, VI_TILE), (unsigned)mud_cdiv(Y, VI_TILE), (unsigned)(s1 - s0 + 1));
  MUD_REQUIRE(grid.y <= 65535 && grid.z <= 65535, "mud_volume_slab_zscore: the volume is too large");
  VI_DISPATCH(datatype, hipLaunchKernelGGL(k_vi_slab_zscore<T>, grid, dim3(VI_THREADS), 0, (hipStream_t)stream,
                                           vi_source_of(vol, datatype, slope, inter), X, Y, s0, mean, std, out));
  MUD_CHECK_LAUNCH("mud_volume_slab_zscore");
  return MUD_OK;
}

// ---- assemble: planes [n][X][Y] -> zero-filled volume [Z][Y][X] with the planes at s0..s1 -------------------------------------------------
__global__ __launch_bounds__(VI_THREADS) void k_vi_assemble(const float* __restrict__ planes, int X, int Y, int s0, int s1,
                                                            float* __restrict__ vol) {
  __shared__ float tile[VI_TILE][VI_TILE + 1];
  const int x0 = blockIdx.x * VI_TILE, y0 = blockIdx.y * VI_TILE, z = blockIdx.z;
  const int l = threadIdx.x & (VI_TILE - 1), r0 = threadIdx.x / VI_TILE;
  const bool inside = z >= s0 && z <= s1;                                   // block-uniform
  if (inside) {
    const float* __restrict__ src = planes + (int64_t)(z - s0) * X * Y;
    for (int r = r0; r < VI_TILE; r += VI_THREADS / VI_TILE) {               // x = x0 + r, lanes along y
      const int x = x0 + r, y = y0 + l;
      if (x < X && y < Y) tile[r][l] = src[(int64_t)x * Y + y];
    }
    __syncthreads();
  }
  float* __restrict__ dst = vol + (int64_t)z * X * Y;
  for (int r = r0; r < VI_TILE; r += VI_THREADS / VI_TILE) {                 // y = y0 + r, lanes along x
    const int x = x0 + l, y = y0 + r;
    if (x < X && y < Y) dst[(int64_t)y * X + x] = inside ? tile[l][r] : 0.0f;
  }
}

extern "C" int mud_volume_assemble(const float* planes, const float* planes2, int X, int Y, int Z, int s0, int s1, float* vol, float* vol2,
                                   void* stream) {
  if (int e = vi_check_size("mud_volume_assemble", "volume", X, Y, Z)) return e;
  MUD_REQUIRE(s0 >= 0 && s1 >= s0 && s1 < Z, "mud_volume_assemble: the slab %d..%d is not inside the %d planes", s0, s1, Z);
  MUD_REQUIRE(planes != nullptr && vol != nullptr, "mud_volume_assemble: null pointer");
  MUD_REQUIRE((planes2 == nullptr) == (vol2 == nullptr), "mud_volume_assemble: the second stack and the second volume go together");
  const dim3 grid((unsigned)mud_cdiv(X, VI_TILE), (unsigned)mud_cdiv(Y, VI_TILE), (unsigned)Z);
  MUD_REQUIRE(grid.y <= 65535 && grid.z <= 65535, "mud_volume_assemble: the volume is too large");
  hipLaunchKernelGGL(k_vi_assemble, grid, dim3(VI_THREADS), 0, (hipStream_t)stream, planes, X, Y, s0, s1, vol);
  MUD_CHECK_LAUNCH("mud_volume_assemble");
  if (planes2) {
    hipLaunchKernelGGL(k_vi_assemble, grid, dim3(VI_THREADS), 0, (hipStream_t)stream, planes2, X, Y, s0, s1, vol2);
    MUD_CHECK_LAUNCH("mud_volume_assemble (second stack)");
  }
  return MUD_OK;
}

// ---- regrid: a volume on another voxel grid -> fp32 [Z][Y][X] on the reference grid ---------------------------------------------------
template <typename T>
__global__ __launch_bounds__(VI_THREADS) void k_vi_regrid(vi_source src, int SX, int SY, int SZ, vi_mat M, int mode, int X, int Y, int64_t n,
                                                          float* __restrict__ out) {
  VI_GRID_STRIDE(i, n) {
    int x, y, z;
    vi_xyz(i, X, Y, x, y, z);
    double p[3];
    vi_coordinate(M, (double)x, (double)y, (double)z, p);
    float r = 0.0f;
    if (mode == 1) {                                         // nearest: floor(p + 0.5) per axis, 0 outside
      const double qx = floor(p[0] + 0.5), qy = floor(p[1] + 0.5), qz = floor(p[2] + 0.5);
      if (qx >= 0.0 && qx < (double)SX && qy >= 0.0 && qy < (double)SY && qz >= 0.0 && qz < (double)SZ)
        r = vi_at<T>(src, ((int64_t)(int)qz * SY + (int)qy) * SX + (int)qx);
    } else if (vi_axis_near(p[0], SX) && vi_axis_near(p[1], SY) && vi_axis_near(p[2], SZ)) {
      r = vi_trilinear<T>(src, SX, SY, SZ, p);
    }
    out[i] = r;
  }
}

extern "C" int mud_volume_regrid(const void* src, int datatype, int SX, int SY, int SZ, float slope, float inter, const double* m, int mode,
                                 int X, int Y, int Z, float* out, void* stream) {
  if (int e = vi_check_volume("mud_volume_regrid", src, datatype, SX, SY, SZ)) return e;
  if (int e = vi_check_size("mud_volume_regrid", "output", X, Y, Z)) return e;
  MUD_REQUIRE(out != nullptr && m != nullptr, "mud_volume_regrid: null pointer");
  MUD_REQUIRE(mode == 0 || mode == 1, "mud_volume_regrid: mode %d is neither 0 (trilinear) nor 1 (nearest)", mode);
  vi_mat M;
  for (int i = 0; i < 12; ++i) {
    MUD_REQUIRE(m[i] - m[i] == 0.0, "mud_volume_regrid: m[%d] = %g is not finite", i, m[i]);
    M.m[i] = m[i];
  }
  const int64_t n = (int64_t)X * Y * Z;
  VI_DISPATCH(datatype, hipLaunchKernelGGL(k_vi_regrid<T>, dim3(vi_blocks(n)), dim3(VI_THREADS), 0, (hipStream_t)stream,
                                           vi_source_of(src, datatype, slope, inter), SX, SY, SZ, M, mode, X, Y, n, out));
  MUD_CHECK_LAUNCH("mud_volume_regrid");
  return MUD_OK;
}
