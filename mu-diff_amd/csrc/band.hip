// Sampling a target given as a thick-slice volume of its own geometry (include/mudiff_hip.h: mud_band_constrain, mud_band_measure;
// mudiff_hip.thick_volume).  Thick slice j is a weighted average of thin slices, y_j = sum_i A_ji k_i per pixel,
// and the thick slices may cut thin slices in fractions or overlap: G = A A^T is a banded SPD matrix and the data-consistency step is the
// orthogonal projection  x <- x - A^T G^-1 (A (x - s eta) - a y)  along z, a banded Cholesky solve per pixel:
//  - forward   j = 0..m-1:  r_j = sum_s w_js (x[member_js] - s eta[member_js]) - a y_j,  v_j = (r_j - sum_k Lc[j][k] v_{j-k}) * dinv_j
//  - backward  j = m-1..0:  u_j = (v_j - sum_k Lc[j+k][k] u_{j+k}) * dinv_j
//  - scatter   every thin slice i:  c = sum_j w_ji u_j,  out_i = x_i - c
// One thread owns one quad (4 consecutive floats = one Philox block of keyed_normal.h) of one set's whole z column and walks the three
// passes alone; v and u live in the caller's workspace, the last bw of them in registers.  No LDS, no atomics, no contraction: sums run
// in the tables' order, so a set's result is a function of its own rows, keys and tables alone.
#include "keyed_rows.h"

#define BD_THREADS 256

// grid (blocks over the row's quads, sets).  MEASURE: out = A x [sets][m][row_len], nothing else is written and y, work are not read.
// Else out may alias x: a thread reads its column of x in the forward pass and again, element by element, just before it writes it.
// The tables sit in device memory (they are too large for kernel arguments); every index read from them is checked against m or n
// before it addresses a row, so a damaged table cannot make the kernel leave its buffers.
template <bool VEC, bool MEASURE>
__global__ __launch_bounds__(BD_THREADS) void k_band(const float* x, const float* __restrict__ y, mud_band_tables tab, keyed_level lv, float* out,
                                                     float* work, int64_t row_len, int64_t quads) {
#pragma clang fp contract(off)   // s * eta, x - ., w * ., acc + ., Lc * v, ...: each rounded once
  const int64_t b = (int64_t)blockIdx.x * BD_THREADS + threadIdx.x;
  if (b >= quads) return;
  const int m = tab.m, nthin = tab.n, bw = tab.bw, ld = tab.bw + 1;
  const int32_t* __restrict__ start = tab.start;
  const int32_t* __restrict__ member = tab.member;
  const float* __restrict__ wt = tab.w;
  const float* __restrict__ lc = tab.lc;
  const int64_t col = 4 * b;
  const int n = VEC ? 4 : (int)(row_len - col < 4 ? row_len - col : 4);
  const int64_t row0 = (int64_t)blockIdx.y * nthin;                       // the set's first row of x, noise, keys and t
  const int64_t wbase = (int64_t)blockIdx.y * m * row_len + col;          // the set's column of work (MEASURE: of out)
  const bool noisy = !MEASURE && !lv.clean;
  float a = 1.f, sg = 0.f;
  if (noisy) {
    const int64_t ti = mud_level_index(lv.t, row0, lv.toff, lv.ntab);     // the level of the set's row 0
    a = lv.at[ti];
    sg = lv.st[ti];
  }
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 hist[MUD_BAND_MAX_BW];                                             // hist[k - 1] = v_{j-k} (backward: u_{j+k})
#pragma unroll
  for (int k = 0; k < MUD_BAND_MAX_BW; ++k) hist[k] = zero;

  for (int j = 0; j < m; ++j) {                                            // ---- forward
    int s0 = start[j], s1 = start[j + 1];
    s0 = s0 < 0 ? 0 : s0;
    s1 = s1 > tab.nnz ? tab.nnz : s1;
    f32x4 acc = zero;
    for (int s = s0; s < s1; ++s) {                                        // table order
      const int i = member[s];
      if ((unsigned)i >= (unsigned)nthin) continue;
      const int64_t base = (row0 + i) * row_len + col;
      f32x4 d = quad_load<VEC>(x + base, n);
      if (noisy) {
        const f32x4 eta = quad_eta<VEC>(lv, row0 + i, (uint64_t)b, base, n);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = sg * eta[e];
          d[e] = d[e] - p;
        }
      }
      const float w = wt[s];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = w * d[e];
        acc[e] = acc[e] + p;
      }
    }
    if constexpr (MEASURE) {
      quad_store<VEC>(out + wbase + (int64_t)j * row_len, acc, n);
    } else {
      const f32x4 yv = quad_load<VEC>(y + (int64_t)j * row_len + col, n);
      f32x4 t = zero;
#pragma unroll
      for (int k = 1; k <= MUD_BAND_MAX_BW; ++k) {
        if (k <= bw && k <= j) {
          const float l = lc[j * ld + k];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float p = l * hist[k - 1][e];
            t[e] = t[e] + p;
          }
        }
      }
      const float dinv = lc[j * ld];
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float ay = noisy ? a * yv[e] : yv[e];
        const float r = acc[e] - ay;
        const float q = r - t[e];
        v[e] = q * dinv;
      }
#pragma unroll
      for (int k = MUD_BAND_MAX_BW - 1; k > 0; --k) hist[k] = hist[k - 1];
      hist[0] = v;
      quad_store<VEC>(work + wbase + (int64_t)j * row_len, v, n);
    }
  }
  if constexpr (!MEASURE) {
#pragma unroll
    for (int k = 0; k < MUD_BAND_MAX_BW; ++k) hist[k] = zero;
    for (int j = m - 1; j >= 0; --j) {                                     // ---- backward, u over v in work
      const f32x4 v = quad_load<VEC>(work + wbase + (int64_t)j * row_len, n);
      f32x4 t = zero;
#pragma unroll
      for (int k = 1; k <= MUD_BAND_MAX_BW; ++k) {
        if (k <= bw && j + k < m) {
          const float l = lc[(j + k) * ld + k];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float p = l * hist[k - 1][e];
            t[e] = t[e] + p;
          }
        }
      }
      const float dinv = lc[j * ld];
      f32x4 u;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float q = v[e] - t[e];
        u[e] = q * dinv;
      }
#pragma unroll
      for (int k = MUD_BAND_MAX_BW - 1; k > 0; --k) hist[k] = hist[k - 1];
      hist[0] = u;
      quad_store<VEC>(work + wbase + (int64_t)j * row_len, u, n);
    }
    const int32_t* __restrict__ tstart = tab.tstart;
    const int32_t* __restrict__ tmember = tab.tmember;
    const float* __restrict__ tw = tab.tw;
    for (int i = 0; i < nthin; ++i) {                                      // ---- scatter: every element of out once, by its owner
      int s0 = tstart[i], s1 = tstart[i + 1];
      s0 = s0 < 0 ? 0 : s0;
      s1 = s1 > tab.nnz ? tab.nnz : s1;
      const int64_t base = (row0 + i) * row_len + col;
      if (s0 >= s1 && out == x) continue;                                  // a row under no thick slice, in place: untouched
      const f32x4 xv = quad_load<VEC>(x + base, n);
      f32x4 c = zero;
      for (int s = s0; s < s1; ++s) {                                      // j ascending
        const int j = tmember[s];
        if ((unsigned)j >= (unsigned)m) continue;
        const f32x4 u = quad_load<VEC>(work + wbase + (int64_t)j * row_len, n);
        const float w = tw[s];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = w * u[e];
          c[e] = c[e] + p;
        }
      }
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = xv[e] - c[e];
        o[e] = c[e] == 0.f ? xv[e] : v;                                    // a correction that is 0 leaves x's bits (a -0 included)
      }
      quad_store<VEC>(out + base, o, n);
    }
  }
}

// [p, p + bytes) and [q, q + qbytes) share a byte
static inline bool bd_overlap(const void* p, int64_t bytes, const void* q, int64_t qbytes) {
  if (!p || !q) return false;
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)qbytes && b < a + (uintptr_t)bytes;
}

static int bd_check(const char* who, const mud_band_tables* tab, int sets, int64_t row_len) {
  MUD_REQUIRE(tab, "%s: null pointer (tab)", who);
  MUD_REQUIRE(tab->m >= 1 && tab->m <= MUD_BAND_MAX_M, "%s: tab.m must be in [1, %d], got %d", who, MUD_BAND_MAX_M, tab->m);
  MUD_REQUIRE(tab->n >= 1 && tab->n <= MUD_BAND_MAX_N, "%s: tab.n must be in [1, %d], got %d", who, MUD_BAND_MAX_N, tab->n);
  MUD_REQUIRE(tab->bw >= 0 && tab->bw <= MUD_BAND_MAX_BW && tab->bw < tab->m, "%s: tab.bw must be in [0, min(%d, m - 1)], got %d", who,
              MUD_BAND_MAX_BW, tab->bw);
  MUD_REQUIRE(tab->nnz >= tab->m && tab->nnz <= tab->m * MUD_BAND_MAX_MEMBERS, "%s: tab.nnz must be in [m, m * %d], got %d", who,
              MUD_BAND_MAX_MEMBERS, tab->nnz);
  MUD_REQUIRE(tab->start && tab->member && tab->w && tab->tstart && tab->tmember && tab->tw && tab->lc, "%s: null pointer in tab", who);
  MUD_REQUIRE(sets > 0 && sets <= 65535 && row_len > 0, "%s: bad sizes (sets %d, row_len %lld)", who, sets, (long long)row_len);
  MUD_REQUIRE((int64_t)sets * tab->n * row_len < (1ll << 31), "%s: sets * n * row_len must be < 2^31, got %d x %d x %lld", who, sets, tab->n,
              (long long)row_len);
  MUD_REQUIRE((int64_t)sets * tab->m * row_len < (1ll << 31), "%s: sets * m * row_len must be < 2^31, got %d x %d x %lld", who, sets, tab->m,
              (long long)row_len);
  return MUD_OK;
}

template <bool MEASURE>
static int bd_run(const char* who, bool vec, const float* x, const float* y, const mud_band_tables& tab, const keyed_level& d, float* out, float* work,
                  int sets, int64_t row_len, void* stream) {
  const int64_t quads = mud_cdiv(row_len, 4);
  vec_dispatch(vec, [&](auto v) {
    hipLaunchKernelGGL((k_band<VEC_OF(v), MEASURE>), dim3((unsigned)mud_cdiv(quads, BD_THREADS), (unsigned)sets), dim3(BD_THREADS), 0, (hipStream_t)stream,
                       x, y, tab, d, out, work, row_len, quads);
  });
  MUD_CHECK_LAUNCH(who);
  return MUD_OK;
}

extern "C" int mud_band_constrain(const float* x, const float* y, const mud_band_tables* tab, const float* noise, const int64_t* keys, uint64_t seed,
                                  int step, int kind, const int64_t* t, int toff, const float* a_tab, const float* s_tab, int ntab, int clean,
                                  float* out, float* work, int sets, int64_t row_len, void* stream) {
  keyed_level d = {noise, keys, seed, 0, t, toff, a_tab, s_tab, ntab, clean};
  MUD_TRY(bd_check("mud_band_constrain", tab, sets, row_len));
  MUD_TRY(keyed_level_word2("mud_band_constrain", ntab, kind, step, d.word2));
  MUD_REQUIRE(x && y && out && work, "mud_band_constrain: null pointer (x, y, out, work)");
  MUD_TRY(keyed_level_operands("mud_band_constrain", true, d));
  const int64_t xb = (int64_t)sets * tab->n * row_len * 4, wb = (int64_t)sets * tab->m * row_len * 4, yb = (int64_t)tab->m * row_len * 4;
  MUD_REQUIRE(!bd_overlap(work, wb, x, xb) && !bd_overlap(work, wb, out, xb) && !bd_overlap(work, wb, y, yb) && !bd_overlap(work, wb, noise, xb),
              "mud_band_constrain: work must not overlap x, y, noise or out");
  MUD_REQUIRE(out == x || !bd_overlap(out, xb, x, xb), "mud_band_constrain: out must be x itself or not overlap it");
  MUD_REQUIRE(!bd_overlap(out, xb, y, yb) && !bd_overlap(out, xb, noise, xb), "mud_band_constrain: out must not overlap y or noise");
  const bool vec = row_len % 4 == 0 && mud_aligned16(x) && mud_aligned16(out) && mud_aligned16(y) && mud_aligned16(work) && (!noise || mud_aligned16(noise));
  return bd_run<false>("mud_band_constrain", vec, x, y, *tab, d, out, work, sets, row_len, stream);
}

extern "C" int mud_band_measure(const float* x, const mud_band_tables* tab, float* ax, int sets, int64_t row_len, void* stream) {
  MUD_TRY(bd_check("mud_band_measure", tab, sets, row_len));
  MUD_REQUIRE(x && ax, "mud_band_measure: null pointer (x, ax)");
  MUD_REQUIRE(!bd_overlap(ax, (int64_t)sets * tab->m * row_len * 4, x, (int64_t)sets * tab->n * row_len * 4), "mud_band_measure: ax must not overlap x");
  const bool vec = row_len % 4 == 0 && mud_aligned16(x) && mud_aligned16(ax);
  const keyed_level none = {nullptr, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, 1, 1};
  return bd_run<true>("mud_band_measure", vec, x, nullptr, *tab, none, ax, nullptr, sets, row_len, stream);
}
