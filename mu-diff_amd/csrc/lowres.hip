// Sampling a target given as a volume that is coarser than the sampled stack in all three axes (include/mudiff_hip.h:
// mud_lowres_constrain, mud_lowres_measure; mudiff_hip.lowres_volume).  A coarse voxel is a separable weighted
// average of fine voxels, A = A_z (x) A_y (x) A_x with every factor banded, so A A^T = G_z (x) G_y (x) G_x and the data-consistency step
//   x <- x - A^T (A A^T)^-1 (A (x - s eta) - a y)
// is three banded Cholesky solves, one per axis, between one gather and one scatter over the full-resolution state:
//  1. in-plane measure  P[r][jy][jx] = sum_yy sum_xx A_y[jy][yy] A_x[jx][xx] (x - s eta)[r][yy][xx]      every row r    (k_lr_inplane)
//  2. z measure, solve  R = A_z P - a y,  U = G_z^-1 R  along jz, per coarse column (jy, jx)             as band.hip   (k_lr_z)
//  3. in-plane solves   U <- G_y^-1 U along jy, then U <- G_x^-1 U along jx, per coarse slice                           (k_lr_plane)
//  4. scatter           out[r][yy][xx] = x - sum_jz sum_jy sum_jx A_z[jz][i] A_y[jy][yy] A_x[jx][xx] U[jz][jy][jx]      (k_lr_scatter)
// Four launches: each pass reads what every workgroup of the one before wrote.  P and U live in the caller's workspace.  No atomics,
// no contraction, every sum from 0 in its table's order: a set's result is a function of its own rows, keys and tables alone.
#include "keyed_rows.h"

#define LR_THREADS 256          // k_lr_plane needs LR_THREADS >= MUD_BAND_MAX_M: one thread per line of a coarse slice
#define LR_MAX_W MUD_BAND_MAX_N // the column sums of one image row in LDS

// a CSR row's [s0, s1), cut to the table
__device__ __forceinline__ void lr_span(const int32_t* __restrict__ start, int j, int nnz, int& s0, int& s1) {
  s0 = start[j];
  s1 = start[j + 1];
  s0 = s0 < 0 ? 0 : s0;
  s1 = s1 > nnz ? nnz : s1;
}

// eta of the 4 elements from `flat` of row r (flat: index within the row of H * W; the Philox block of element e is e / 4, so a quad of
// an image row is one block when W % 4 == 0 and straddles two otherwise)
template <bool VEC>
__device__ __forceinline__ f32x4 lr_eta(const keyed_level& d, int64_t r, int64_t row_len, int64_t flat, int n) {
  if (d.noise) return quad_load<VEC>(d.noise + r * row_len + flat, n);
  const uint64_t k0 = (uint64_t)d.keys[2 * r], k1 = (uint64_t)d.keys[2 * r + 1];
  const f32x4 e0 = es_block_normals((uint64_t)(flat >> 2), k0, k1, d.seed, d.word2);
  if constexpr (VEC) return e0;
  const int o = (int)(flat & 3);
  if (o == 0) return e0;
  const f32x4 e1 = es_block_normals((uint64_t)(flat >> 2) + 1, k0, k1, d.seed, d.word2);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int k = 0; k < 7; ++k)                       // selects with constant lanes: no indexed register access
      if (o + e == k) v[e] = k < 4 ? e0[k & 3] : e1[k & 3];
  return v;
}

// ---- 1. grid (m_y, rows): the workgroup of (jy, r) adds the image rows under coarse row jy per column (a thread owns quads of columns,
// table order along y, in registers), leaves the W column sums in LDS and then adds them along x, one thread per coarse column jx.
template <bool VEC>
__global__ __launch_bounds__(LR_THREADS) void k_lr_inplane(const float* __restrict__ x, mud_band_tables ty, mud_band_tables tx, keyed_level lv, int nz,
                                                           float* __restrict__ P, int H, int W) {
#pragma clang fp contract(off)
  __shared__ float cols[LR_MAX_W];
  const int jy = blockIdx.x;
  const int64_t r = blockIdx.y;
  const int64_t row_len = (int64_t)H * W;
  const bool noisy = !lv.clean;
  float sg = 0.f;
  if (noisy) sg = lv.st[mud_level_index(lv.t, r / nz * nz, lv.toff, lv.ntab)];      // the level of the set's row 0
  int y0, y1;
  lr_span(ty.start, jy, ty.nnz, y0, y1);
  const int quads = (W + 3) >> 2;
  for (int q = threadIdx.x; q < quads; q += LR_THREADS) {
    const int n = VEC ? 4 : (W - 4 * q < 4 ? W - 4 * q : 4);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = y0; s < y1; ++s) {                                                   // table order
      const int yy = ty.member[s];
      if ((unsigned)yy >= (unsigned)H) continue;
      const int64_t flat = (int64_t)yy * W + 4 * q;
      f32x4 d = quad_load<VEC>(x + r * row_len + flat, n);
      if (noisy) {
        const f32x4 eta = lr_eta<VEC>(lv, r, row_len, flat, n);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = sg * eta[e];
          d[e] = d[e] - p;
        }
      }
      const float w = ty.w[s];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = w * d[e];
        acc[e] = acc[e] + p;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < n) cols[4 * q + e] = acc[e];
  }
  __syncthreads();
  for (int jx = threadIdx.x; jx < tx.m; jx += LR_THREADS) {
    int s0, s1;
    lr_span(tx.start, jx, tx.nnz, s0, s1);
    float acc = 0.f;
    for (int s = s0; s < s1; ++s) {                                                   // table order
      const int xx = tx.member[s];
      if ((unsigned)xx >= (unsigned)W) continue;
      const float p = tx.w[s] * cols[xx];
      acc = acc + p;
    }
    P[(r * ty.m + jy) * tx.m + jx] = acc;
  }
}

// the banded solves: hist[k - 1] = the value k steps back along the sweep
__device__ __forceinline__ float lr_back_sum(const float* __restrict__ lc, int ld, int bw, int row_of_k1, int step, int avail, const float (&hist)[MUD_BAND_MAX_BW]) {
#pragma clang fp contract(off)
  // forward: row j's entries lc[j][k] (row_of_k1 = j, step = 0); backward: lc[j + k][k] (row_of_k1 = j + 1, step = 1); k <= avail
  float t = 0.f;
#pragma unroll
  for (int k = 1; k <= MUD_BAND_MAX_BW; ++k) {
    if (k <= bw && k <= avail) {
      const float p = lc[(row_of_k1 + step * (k - 1)) * ld + k] * hist[k - 1];
      t = t + p;
    }
  }
  return t;
}

__device__ __forceinline__ void lr_push(float (&hist)[MUD_BAND_MAX_BW], float v) {
#pragma unroll
  for (int k = MUD_BAND_MAX_BW - 1; k > 0; --k) hist[k] = hist[k - 1];
  hist[0] = v;
}

// G^-1 along a line of m values `stride` apart, in place: forward v_j = (u_j - sum_k lc[j][k] v_{j-k}) * lc[j][0], then backward
__device__ __forceinline__ void lr_solve_line(float* u, int64_t stride, const mud_band_tables& tab) {
#pragma clang fp contract(off)
  const int m = tab.m, bw = tab.bw, ld = tab.bw + 1;
  const float* __restrict__ lc = tab.lc;
  float hist[MUD_BAND_MAX_BW];
#pragma unroll
  for (int k = 0; k < MUD_BAND_MAX_BW; ++k) hist[k] = 0.f;
  for (int j = 0; j < m; ++j) {
    const float t = lr_back_sum(lc, ld, bw, j, 0, j, hist);
    const float q = u[j * stride] - t;
    const float v = q * lc[j * ld];
    lr_push(hist, v);
    u[j * stride] = v;
  }
#pragma unroll
  for (int k = 0; k < MUD_BAND_MAX_BW; ++k) hist[k] = 0.f;
  for (int j = m - 1; j >= 0; --j) {
    const float t = lr_back_sum(lc, ld, bw, j + 1, 1, m - 1 - j, hist);
    const float q = u[j * stride] - t;
    const float v = q * lc[j * ld];
    lr_push(hist, v);
    u[j * stride] = v;
  }
}

// ---- 2. grid (blocks over the L = m_y * m_x coarse columns, sets): band.hip's forward and backward passes on P, one thread per coarse
// column.  MEASURE: out = A_z P [sets][m_z][L] and nothing else.
template <bool MEASURE>
__global__ __launch_bounds__(LR_THREADS) void k_lr_z(const float* __restrict__ P, const float* __restrict__ y, mud_band_tables tz, keyed_level lv,
                                                     float* __restrict__ U, int64_t L) {
#pragma clang fp contract(off)
  const int64_t c = (int64_t)blockIdx.x * LR_THREADS + threadIdx.x;
  if (c >= L) return;
  const int m = tz.m, nz = tz.n;
  const int64_t row0 = (int64_t)blockIdx.y * nz;
  float* u = U + (int64_t)blockIdx.y * m * L + c;
  const bool noisy = !MEASURE && !lv.clean;
  float a = 1.f;
  if (noisy) a = lv.at[mud_level_index(lv.t, row0, lv.toff, lv.ntab)];
  for (int j = 0; j < m; ++j) {
    int s0, s1;
    lr_span(tz.start, j, tz.nnz, s0, s1);
    float acc = 0.f;
    for (int s = s0; s < s1; ++s) {                                                   // table order
      const int i = tz.member[s];
      if ((unsigned)i >= (unsigned)nz) continue;
      const float p = tz.w[s] * P[(row0 + i) * L + c];
      acc = acc + p;
    }
    if constexpr (!MEASURE) {
      const float yv = y[(int64_t)j * L + c];
      const float ay = noisy ? a * yv : yv;
      acc = acc - ay;
    }
    u[(int64_t)j * L] = acc;
  }
  if constexpr (!MEASURE) lr_solve_line(u, L, tz);
}

// ---- 3. grid (m_z, sets): one workgroup per coarse slice, one thread per line.  The y solve runs down the columns, thread = jx, so a
// wave's accesses are consecutive; the x solve runs along the rows, thread = jy, straight from L2 (a slice is at most 256 KiB and was
// written by this workgroup a moment ago; staging it would need more LDS than a tile of lines saves).
__global__ __launch_bounds__(LR_THREADS) void k_lr_plane(float* U, mud_band_tables ty, mud_band_tables tx) {
  float* u = U + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * ty.m * tx.m;
  for (int jx = threadIdx.x; jx < tx.m; jx += LR_THREADS) lr_solve_line(u + jx, tx.m, ty);
  __syncthreads();
  for (int jy = threadIdx.x; jy < ty.m; jy += LR_THREADS) lr_solve_line(u + (int64_t)jy * tx.m, 1, tx);
}

// ---- 4. one thread per quad of out, with the transposed tables: c = sum_jz tw_z (sum_jy tw_y (sum_jx tw_x U)), each sum from 0 with
// its index ascending.  In place a quad under no coarse voxel is not touched; an element whose correction is 0 keeps x's bits.
template <bool VEC>
__global__ __launch_bounds__(LR_THREADS) void k_lr_scatter(const float* x, const float* __restrict__ U, mud_band_tables tz, mud_band_tables ty,
                                                           mud_band_tables tx, float* out, int rows, int H, int W) {
#pragma clang fp contract(off)
  const int quads = (W + 3) >> 2;
  const int64_t tid = (int64_t)blockIdx.x * LR_THREADS + threadIdx.x;
  if (tid >= (int64_t)rows * H * quads) return;
  const int q = (int)(tid % quads);
  const int yy = (int)(tid / quads % H);
  const int64_t r = tid / quads / H;
  const int i = (int)(r % tz.n);
  const int64_t set = r / tz.n;
  const int n = VEC ? 4 : (W - 4 * q < 4 ? W - 4 * q : 4);
  const int64_t base = (r * H + yy) * W + 4 * q;
  int z0, z1, y0, y1, x0[4], x1[4];
  lr_span(tz.tstart, i, tz.nnz, z0, z1);
  lr_span(ty.tstart, yy, ty.nnz, y0, y1);
  bool any = false;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    x0[e] = x1[e] = 0;
    if (e < n) lr_span(tx.tstart, 4 * q + e, tx.nnz, x0[e], x1[e]);
    any = any || x0[e] < x1[e];
  }
  const bool covered = z0 < z1 && y0 < y1 && any;
  if (!covered && out == x) return;
  const f32x4 xv = quad_load<VEC>(x + base, n);
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  if (covered) {
    const int64_t L = (int64_t)ty.m * tx.m;
    for (int sz = z0; sz < z1; ++sz) {                                                // jz ascending
      const int jz = tz.tmember[sz];
      if ((unsigned)jz >= (unsigned)tz.m) continue;
      const float* __restrict__ uz = U + (set * tz.m + jz) * L;
      f32x4 cy = {0.f, 0.f, 0.f, 0.f};
      for (int sy = y0; sy < y1; ++sy) {                                              // jy ascending
        const int jy = ty.tmember[sy];
        if ((unsigned)jy >= (unsigned)ty.m) continue;
        const float* __restrict__ uy = uz + (int64_t)jy * tx.m;
        const float wy = ty.tw[sy];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float cx = 0.f;
          for (int sx = x0[e]; sx < x1[e]; ++sx) {                                    // jx ascending
            const int jx = tx.tmember[sx];
            if ((unsigned)jx >= (unsigned)tx.m) continue;
            const float p = tx.tw[sx] * uy[jx];
            cx = cx + p;
          }
          const float p = wy * cx;
          cy[e] = cy[e] + p;
        }
      }
      const float wz = tz.tw[sz];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = wz * cy[e];
        c[e] = c[e] + p;
      }
    }
  }
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float v = xv[e] - c[e];
    o[e] = c[e] == 0.f ? xv[e] : v;                                                   // a correction that is 0 leaves x's bits (a -0 included)
  }
  quad_store<VEC>(out + base, o, n);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static inline bool lr_overlap(const void* p, int64_t bytes, const void* q, int64_t qbytes) {
  if (!p || !q) return false;
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)qbytes && b < a + (uintptr_t)bytes;
}

static int lr_check_axis(const char* who, const char* axis, const mud_band_tables* tab) {
  MUD_REQUIRE(tab, "%s: null pointer (tab_%s)", who, axis);
  MUD_REQUIRE(tab->m >= 1 && tab->m <= MUD_BAND_MAX_M, "%s: tab_%s.m must be in [1, %d], got %d", who, axis, MUD_BAND_MAX_M, tab->m);
  MUD_REQUIRE(tab->n >= 1 && tab->n <= MUD_BAND_MAX_N, "%s: tab_%s.n must be in [1, %d], got %d", who, axis, MUD_BAND_MAX_N, tab->n);
  MUD_REQUIRE(tab->bw >= 0 && tab->bw <= MUD_BAND_MAX_BW && tab->bw < tab->m, "%s: tab_%s.bw must be in [0, min(%d, m - 1)], got %d", who, axis,
              MUD_BAND_MAX_BW, tab->bw);
  MUD_REQUIRE(tab->nnz >= tab->m && tab->nnz <= tab->m * MUD_BAND_MAX_MEMBERS, "%s: tab_%s.nnz must be in [m, m * %d], got %d", who, axis,
              MUD_BAND_MAX_MEMBERS, tab->nnz);
  MUD_REQUIRE(tab->start && tab->member && tab->w && tab->tstart && tab->tmember && tab->tw && tab->lc, "%s: null pointer in tab_%s", who, axis);
  return MUD_OK;
}

static int lr_check(const char* who, const mud_band_tables* tz, const mud_band_tables* ty, const mud_band_tables* tx, int H, int W, int rows) {
  MUD_TRY(lr_check_axis(who, "z", tz));
  MUD_TRY(lr_check_axis(who, "y", ty));
  MUD_TRY(lr_check_axis(who, "x", tx));
  MUD_REQUIRE(H >= 1 && W >= 1 && rows >= 1, "%s: bad sizes (H %d, W %d, rows %d)", who, H, W, rows);
  MUD_REQUIRE(ty->n == H, "%s: tab_y.n must be H = %d, got %d", who, H, ty->n);
  MUD_REQUIRE(tx->n == W, "%s: tab_x.n must be W = %d, got %d", who, W, tx->n);
  MUD_REQUIRE(rows % tz->n == 0, "%s: tab_z.n = %d must divide the %d rows", who, tz->n, rows);
  MUD_REQUIRE(rows <= 65535, "%s: at most 65535 rows, got %d", who, rows);
  MUD_REQUIRE((int64_t)rows * H * W < (1ll << 31), "%s: rows * H * W must be < 2^31, got %d x %d x %d", who, rows, H, W);
  return MUD_OK;
}

extern "C" int64_t mud_lowres_ws_floats(int sets, int n, int m_z, int m_y, int m_x) {
  if (sets < 1 || n < 1 || m_z < 1 || m_y < 1 || m_x < 1) return -1;
  return ((int64_t)sets * n + (int64_t)sets * m_z) * m_y * m_x;
}

// P: work [rows][m_y][m_x];  U: behind it, [sets][m_z][m_y][m_x]
template <bool MEASURE>
static int lr_run(const char* who, const float* x, const float* y, const mud_band_tables& tz, const mud_band_tables& ty, const mud_band_tables& tx,
                  const keyed_level& d, float* out, float* work, int H, int W, int rows, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const int sets = rows / tz.n;
  const int64_t L = (int64_t)ty.m * tx.m;
  float* P = work;
  float* U = work + (int64_t)rows * L;
  const bool vec = W % 4 == 0 && mud_aligned16(x) && (MEASURE || mud_aligned16(out)) && (!d.noise || mud_aligned16(d.noise));
  vec_dispatch(vec, [&](auto v) {
    hipLaunchKernelGGL((k_lr_inplane<VEC_OF(v)>), dim3((unsigned)ty.m, (unsigned)rows), dim3(LR_THREADS), 0, st, x, ty, tx, d, tz.n, P, H, W);
  });
  MUD_CHECK_LAUNCH(who);
  hipLaunchKernelGGL((k_lr_z<MEASURE>), dim3((unsigned)mud_cdiv(L, LR_THREADS), (unsigned)sets), dim3(LR_THREADS), 0, st, P, y, tz, d, MEASURE ? out : U, L);
  MUD_CHECK_LAUNCH(who);
  if constexpr (!MEASURE) {
    hipLaunchKernelGGL(k_lr_plane, dim3((unsigned)tz.m, (unsigned)sets), dim3(LR_THREADS), 0, st, U, ty, tx);
    MUD_CHECK_LAUNCH(who);
    const int64_t threads = (int64_t)rows * H * mud_cdiv(W, 4);
    vec_dispatch(vec, [&](auto v) {
      hipLaunchKernelGGL((k_lr_scatter<VEC_OF(v)>), dim3((unsigned)mud_cdiv(threads, LR_THREADS)), dim3(LR_THREADS), 0, st, x, U, tz, ty, tx, out, rows, H, W);
    });
    MUD_CHECK_LAUNCH(who);
  }
  return MUD_OK;
}

extern "C" int mud_lowres_constrain(const float* x, const float* y, const mud_band_tables* tab_z, const mud_band_tables* tab_y,
                                    const mud_band_tables* tab_x, int H, int W, int rows, float* work, const float* noise, const int64_t* keys,
                                    uint64_t seed, int step, int kind, const int64_t* t, int toff, const float* a_tab, const float* s_tab, int ntab,
                                    int clean, float* out, void* stream) {
  static_assert(LR_THREADS >= MUD_BAND_MAX_M && LR_MAX_W >= MUD_BAND_MAX_N, "one thread per line, one LDS float per column");
  keyed_level d = {noise, keys, seed, 0, t, toff, a_tab, s_tab, ntab, clean};
  MUD_TRY(lr_check("mud_lowres_constrain", tab_z, tab_y, tab_x, H, W, rows));
  MUD_TRY(keyed_level_word2("mud_lowres_constrain", ntab, kind, step, d.word2));
  MUD_REQUIRE(x && y && out && work, "mud_lowres_constrain: null pointer (x, y, out, work)");
  MUD_TRY(keyed_level_operands("mud_lowres_constrain", true, d));
  const int64_t L = (int64_t)tab_y->m * tab_x->m;
  const int64_t xb = (int64_t)rows * H * W * 4, yb = (int64_t)tab_z->m * L * 4;
  const int64_t wb = mud_lowres_ws_floats(rows / tab_z->n, tab_z->n, tab_z->m, tab_y->m, tab_x->m) * 4;
  MUD_REQUIRE(!lr_overlap(work, wb, x, xb) && !lr_overlap(work, wb, out, xb) && !lr_overlap(work, wb, y, yb) && !lr_overlap(work, wb, noise, xb),
              "mud_lowres_constrain: work must not overlap x, y, noise or out");
  MUD_REQUIRE(out == x || !lr_overlap(out, xb, x, xb), "mud_lowres_constrain: out must be x itself or not overlap it");
  MUD_REQUIRE(!lr_overlap(out, xb, y, yb) && !lr_overlap(out, xb, noise, xb), "mud_lowres_constrain: out must not overlap y or noise");
  return lr_run<false>("mud_lowres_constrain", x, y, *tab_z, *tab_y, *tab_x, d, out, work, H, W, rows, stream);
}

extern "C" int mud_lowres_measure(const float* x, const mud_band_tables* tab_z, const mud_band_tables* tab_y, const mud_band_tables* tab_x, int H, int W,
                                  int rows, float* work, float* ax, void* stream) {
  MUD_TRY(lr_check("mud_lowres_measure", tab_z, tab_y, tab_x, H, W, rows));
  MUD_REQUIRE(x && ax && work, "mud_lowres_measure: null pointer (x, ax, work)");
  const int64_t L = (int64_t)tab_y->m * tab_x->m;
  const int64_t xb = (int64_t)rows * H * W * 4, ab = (int64_t)(rows / tab_z->n) * tab_z->m * L * 4, wb = (int64_t)rows * L * 4;
  MUD_REQUIRE(!lr_overlap(work, wb, x, xb) && !lr_overlap(work, wb, ax, ab) && !lr_overlap(ax, ab, x, xb), "mud_lowres_measure: x, work and ax must not overlap");
  const keyed_level none = {nullptr, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, 1, 1};
  return lr_run<true>("mud_lowres_measure", x, nullptr, *tab_z, *tab_y, *tab_x, none, ax, work, H, W, rows, stream);
}
