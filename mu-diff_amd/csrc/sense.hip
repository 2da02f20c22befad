// Sampling a target that was acquired accelerated on several coils (include/mudiff_hip.h: mud_sense_constrain, mud_sense_measure,
// mud_sense_adjoint, mud_sense_ws_floats; mudiff_hip.sense).  A x = (M F(C_c x))_c with C the coil sensitivities,
// F kspace.hip's unitary 2D DFT and M the sampling mask; N = A^H A = Re sum_c conj(C_c) F^H M F C_c is dense, so the data-consistency step
// is a proximal one, x = x_new - lambda e with (I + lambda N) e = N (x_new - s eta) - a A^H y solved by `iters` conjugate-gradient steps.
//  - one application of N is three launches, the shape of kspace.hip's three: rows forward (the multiply by C_c, and the vector the
//    application is of, fused into the load), columns forward -> mask -> columns inverse without leaving LDS, rows inverse (a workgroup
//    owns its lines of one slice, loops over the coils and sums Re(conj(C_c) .) in registers; the CG epilogue of that application and
//    its partial of the dot product fused into the store);
//  - every CG scalar is per row and stays on the device: each workgroup sums the row's partials [row][tile] in tile order, so a row
//    alone has the bits it has inside any batch; no atomics.
// A row whose b is exactly 0, whose residual reaches exactly 0 or whose p.q is 0 is frozen: its partials of r.r are written as 0 from
// then on, which every later launch reads as alpha = beta = 0.
#include "keyed_rows.h"
#include "kspace_lines.h"

#pragma clang fp contract(off)   // every product and sum rounds once, as tests/sense_ref.py states them

#define SN_MAX_COILS MUD_SENSE_MAX_COILS
#define SN_MAX_ITERS 64
#define SN_QUADS 4               // quads of 4 elements a thread owns of its workgroup's lines: lines * S / 4 / KS_THREADS <= 4

// what the row passes and the update need beside the lines.  The vectors r, p, q, e are [rows][S][S]; the partials [rows][tiles]
struct sn_con {
  const float* x_new;
  const float* ahy;
  const float2* maps;
  int map_rows, coils;
  float lambda;
  keyed_level d;
  float *r, *p, *q, *e;
  float *bb, *rr_cur, *rr_nxt, *pq;     // partials: |b|^2, r.r of this and of the next iteration, p.q
  float* out;
};

__device__ __forceinline__ double sn_row_sum(const float* part, int64_t r, int tiles) {
  double s = 0.0;
  for (int i = 0; i < tiles; ++i) s += (double)part[r * tiles + i];
  return s;
}

// the sum of v over the workgroup, the same in every thread: 64-lane butterflies, then the 4 waves in order
__device__ __forceinline__ float sn_block_sum(float v) {
  __shared__ float red[KS_THREADS / 64];
  v = mud_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

enum { SN_FWD_PLAIN = 0, SN_FWD_FIRST = 1, SN_FWD_P_INIT = 2, SN_FWD_P_NEXT = 3 };

// Rows forward: workgroup b owns the lines b * L .. b * L + L - 1 of the rows * S lines of the batch (L divides S: one slice r).  It forms
// its lines of the real vector d once, in registers, then per coil c: d * C_c -> forward DIF -> data[r][c], natural order.
//  SN_FWD_PLAIN:  d = in                                   (mud_sense_measure)
//  SN_FWD_FIRST:  d = x_new - s * eta (clean: x_new), a thread's quad = one Philox block, as in k_ks_rows
//  SN_FWD_P_INIT: d = p = r                                (the first CG iteration)
//  SN_FWD_P_NEXT: d = p = r + beta * p, beta = r.r of this iteration / r.r of the one before, 0 for a frozen row
template <int MODE>
__global__ __launch_bounds__(KS_THREADS) void k_sn_rows_fwd(const float* in, float2* data, sn_con c, int logS, int logL) {
  extern __shared__ float2 ks_lds[];
  const int S = 1 << logS, P = S + 1, L = 1 << logL, nq = L << (logS - 2);
  float2* x = ks_lds;
  float2* tw = ks_lds + L * P;
  const int64_t line0 = (int64_t)blockIdx.x << logL, r = line0 >> logS;
  ks_twiddles(tw, S);
  float beta = 0.f;
  if constexpr (MODE == SN_FWD_P_NEXT) {
    const int tiles = S >> logL;
    const double now = sn_row_sum(c.rr_cur, r, tiles), before = sn_row_sum(c.rr_nxt, r, tiles);   // rr_nxt: the buffer this iteration overwrites
    if (now != 0.0 && before != 0.0) beta = (float)now / (float)before;
  }
  f32x4 d[SN_QUADS];
#pragma unroll
  for (int j = 0; j < SN_QUADS; ++j) {
    const int i = threadIdx.x + j * KS_THREADS;
    d[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (i < nq) {
      const int l = i >> (logS - 2), c4 = i & ((S >> 2) - 1);
      const int64_t line = line0 + l, u = line & (S - 1);
      const int64_t g = (line << logS) + 4 * c4;
      if constexpr (MODE == SN_FWD_PLAIN) {
        d[j] = quad_load<true>(in + g, 4);
      } else if constexpr (MODE == SN_FWD_FIRST) {
        d[j] = quad_load<true>(c.x_new + g, 4);
        if (!c.d.clean) {
          const float s = c.d.st[mud_level_index(c.d.t, r, c.d.toff, c.d.ntab)];
          const f32x4 eta = quad_eta<true>(c.d, r, (uint64_t)((u << (logS - 2)) + c4), g, 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float p = s * eta[e];
            d[j][e] = d[j][e] - p;
          }
        }
      } else {
        d[j] = quad_load<true>(c.r + g, 4);
        if constexpr (MODE == SN_FWD_P_NEXT) {
          const f32x4 p = quad_load<true>(c.p + g, 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float bp = beta * p[e];
            d[j][e] = d[j][e] + bp;
          }
        }
        quad_store<true>(c.p + g, d[j], 4);
      }
    }
  }
  const float2* maps = c.maps + (c.map_rows == 1 ? 0 : (r * c.coils) << (2 * logS));
  for (int coil = 0; coil < c.coils; ++coil) {
    const float2* cm = maps + ((int64_t)coil << (2 * logS)) + ((line0 & (S - 1)) << logS);
#pragma unroll
    for (int j = 0; j < SN_QUADS; ++j) {
      const int i = threadIdx.x + j * KS_THREADS;
      if (i < nq) {
        const int l = i >> (logS - 2), c4 = i & ((S >> 2) - 1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float2 m = cm[(l << logS) + 4 * c4 + e];
          x[l * P + 4 * c4 + e] = make_float2(d[j][e] * m.x, d[j][e] * m.y);
        }
      }
    }
    ks_lines_dif(x, P, logL, logS, tw, false);
    float2* dst = data + (((r * c.coils + coil) << (2 * logS)) + ((line0 & (S - 1)) << logS));
    for (int i = threadIdx.x; i < L * S; i += KS_THREADS) {
      const int l = i >> logS, v = i & (S - 1);
      dst[(l << logS) + v] = x[l * P + ks_bitrev(v, logS)];
    }
    __syncthreads();          // the next coil's fill overwrites what the store has just read
  }
}

enum { SN_COL_NORMAL = 0, SN_COL_MEASURE = 1 };

// Column pass over the rows * coils slices of data, in place; workgroup b owns the columns c0 .. c0 + L - 1 of one slice, one per LDS line.
//  SN_COL_NORMAL:  forward DIF, . / S, zero where the mask is 0 (position p = frequency bitrev(p)), inverse DIT, . / S: k_ks_cols<true>
//                  without a y
//  SN_COL_MEASURE: forward DIF, . / S, zero where the mask is 0, stored in natural order
template <int MODE>
__global__ __launch_bounds__(KS_THREADS) void k_sn_cols(float2* data, const uint8_t* __restrict__ mask, int mask_rows, int coils, int logS, int logL) {
  extern __shared__ float2 ks_lds[];
  const int S = 1 << logS, P = S + 1, L = 1 << logL;
  float2* x = ks_lds;
  float2* tw = ks_lds + L * P;
  const int tiles = S >> logL;
  const int64_t sl = blockIdx.x / tiles, r = sl / coils;
  const int c0 = (int)(blockIdx.x - sl * tiles) << logL;
  const float inv_s = 1.0f / (float)S;
  float2* slice = data + (sl << (2 * logS));
  const uint8_t* m = mask + (mask_rows == 1 ? 0 : (r << (2 * logS)));
  ks_twiddles(tw, S);
  for (int i = threadIdx.x; i < L * S; i += KS_THREADS) {
    const int l = i & (L - 1), u = i >> logL;
    x[l * P + u] = slice[(u << logS) + c0 + l];
  }
  ks_lines_dif(x, P, logL, logS, tw, false);
  if constexpr (MODE == SN_COL_NORMAL) {
    for (int i = threadIdx.x; i < L * S; i += KS_THREADS) {
      const int l = i & (L - 1), p = i >> logL;
      const float2 D = x[l * P + p];
      x[l * P + p] = m[(ks_bitrev(p, logS) << logS) + c0 + l] ? make_float2(D.x * inv_s, D.y * inv_s) : make_float2(0.f, 0.f);
    }
    ks_lines_dit(x, P, logL, logS, tw, true);
    for (int i = threadIdx.x; i < L * S; i += KS_THREADS) {
      const int l = i & (L - 1), u = i >> logL;
      const float2 v = x[l * P + u];
      slice[(u << logS) + c0 + l] = make_float2(v.x * inv_s, v.y * inv_s);
    }
  } else {
    for (int i = threadIdx.x; i < L * S; i += KS_THREADS) {
      const int l = i & (L - 1), u = i >> logL;
      const float2 v = x[l * P + ks_bitrev(u, logS)];
      slice[(u << logS) + c0 + l] = m[(u << logS) + c0 + l] ? make_float2(v.x * inv_s, v.y * inv_s) : make_float2(0.f, 0.f);
    }
  }
}

enum { SN_INV_ADJOINT = 0, SN_INV_FIRST = 1, SN_INV_CG = 2 };

// Rows inverse: workgroup b owns its lines of slice r as k_sn_rows_fwd does, loops over the coils (data[r][c] -> inverse DIT) and sums
// acc = sum_c Re(conj(C_c) .) in registers, coil 0 first.  Then, per element,
//  SN_INV_ADJOINT: out = acc                                           (mud_sense_adjoint)
//  SN_INV_FIRST:   r = b = acc - a * ahy,  partials bb = rr_cur = sum b * b of the workgroup's lines
//  SN_INV_CG:      q = p + lambda * acc,   partial pq = sum p * q
template <int MODE>
__global__ __launch_bounds__(KS_THREADS) void k_sn_rows_inv(const float2* data, sn_con c, int logS, int logL) {
  extern __shared__ float2 ks_lds[];
  const int S = 1 << logS, P = S + 1, L = 1 << logL, nq = L << (logS - 2);
  float2* x = ks_lds;
  float2* tw = ks_lds + L * P;
  const int64_t line0 = (int64_t)blockIdx.x << logL, r = line0 >> logS;
  ks_twiddles(tw, S);
  f32x4 acc[SN_QUADS];
#pragma unroll
  for (int j = 0; j < SN_QUADS; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float2* maps = c.maps + (c.map_rows == 1 ? 0 : (r * c.coils) << (2 * logS));
  for (int coil = 0; coil < c.coils; ++coil) {
    const int64_t off = ((int64_t)coil << (2 * logS)) + ((line0 & (S - 1)) << logS);
    const float2* src = data + (((r * c.coils) << (2 * logS)) + off);
    const float2* cm = maps + off;
    for (int i = threadIdx.x; i < L * S; i += KS_THREADS) {
      const int l = i >> logS, v = i & (S - 1);
      x[l * P + ks_bitrev(v, logS)] = src[(l << logS) + v];
    }
    ks_lines_dit(x, P, logL, logS, tw, true);
#pragma unroll
    for (int j = 0; j < SN_QUADS; ++j) {
      const int i = threadIdx.x + j * KS_THREADS;
      if (i < nq) {
        const int l = i >> (logS - 2), c4 = i & ((S >> 2) - 1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float2 m = cm[(l << logS) + 4 * c4 + e], v = x[l * P + 4 * c4 + e];
          const float a = m.x * v.x, b = m.y * v.y;
          const float re = a + b;
          acc[j][e] = acc[j][e] + re;
        }
      }
    }
    __syncthreads();          // the next coil's load overwrites what the sum has just read
  }
  float a = 1.0f;
  if constexpr (MODE == SN_INV_FIRST)
    if (!c.d.clean) a = c.d.at[mud_level_index(c.d.t, r, c.d.toff, c.d.ntab)];
  float dot = 0.f;
#pragma unroll
  for (int j = 0; j < SN_QUADS; ++j) {
    const int i = threadIdx.x + j * KS_THREADS;
    if (i < nq) {
      const int l = i >> (logS - 2), c4 = i & ((S >> 2) - 1);
      const int64_t g = ((line0 + l) << logS) + 4 * c4;
      if constexpr (MODE == SN_INV_ADJOINT) {
        quad_store<true>(c.out + g, acc[j], 4);
      } else if constexpr (MODE == SN_INV_FIRST) {
        const f32x4 h = quad_load<true>(c.ahy + g, 4);
        f32x4 b;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float ah = a * h[e];
          b[e] = acc[j][e] - ah;
          const float sq = b[e] * b[e];
          dot = dot + sq;
        }
        quad_store<true>(c.r + g, b, 4);
      } else {
        const f32x4 p = quad_load<true>(c.p + g, 4);
        f32x4 q;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float ln = c.lambda * acc[j][e];
          q[e] = p[e] + ln;
          const float pq = p[e] * q[e];
          dot = dot + pq;
        }
        quad_store<true>(c.q + g, q, 4);
      }
    }
  }
  if constexpr (MODE != SN_INV_ADJOINT) {
    dot = sn_block_sum(dot);
    if (threadIdx.x == 0) {
      if constexpr (MODE == SN_INV_FIRST) {
        c.bb[blockIdx.x] = dot;
        c.rr_cur[blockIdx.x] = dot;
      } else {
        c.pq[blockIdx.x] = dot;
      }
    }
  }
}

// The vector update of one CG iteration, on the tiling of the row passes: alpha = r.r / p.q (0 for a frozen row), e += alpha p (`first`:
// e = alpha p), r -= alpha q, partial rr_nxt = sum r * r, written as 0 for a frozen row; `last`: out = x_new - lambda e, x_new's bits
// where lambda e compares equal to 0 (out may be x_new: read, then written, by the same thread).
__global__ __launch_bounds__(KS_THREADS) void k_sn_update(sn_con c, int logS, int logL, int first, int last) {
  const int S = 1 << logS, nq = (1 << logL) << (logS - 2), tiles = S >> logL;
  const int64_t line0 = (int64_t)blockIdx.x << logL, r = line0 >> logS;
  const double rr = sn_row_sum(c.rr_cur, r, tiles), pq = sn_row_sum(c.pq, r, tiles);
  const bool frozen = rr == 0.0 || pq == 0.0;
  const float alpha = frozen ? 0.f : (float)rr / (float)pq;
  float dot = 0.f;
  for (int i = threadIdx.x; i < nq; i += KS_THREADS) {
    const int64_t g = (line0 << logS) + 4 * (int64_t)i;
    const f32x4 p = quad_load<true>(c.p + g, 4), q = quad_load<true>(c.q + g, 4);
    f32x4 e = {0.f, 0.f, 0.f, 0.f}, res = quad_load<true>(c.r + g, 4);
    if (!first) e = quad_load<true>(c.e + g, 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float ap = alpha * p[k], aq = alpha * q[k];
      e[k] = e[k] + ap;
      res[k] = res[k] - aq;
      const float sq = res[k] * res[k];
      dot = dot + sq;
    }
    quad_store<true>(c.e + g, e, 4);
    quad_store<true>(c.r + g, res, 4);
    if (last) {
      f32x4 o = quad_load<true>(c.x_new + g, 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float le = c.lambda * e[k];
        o[k] = le == 0.f ? o[k] : o[k] - le;
      }
      quad_store<true>(c.out + g, o, 4);
    }
  }
  dot = sn_block_sum(dot);
  if (threadIdx.x == 0) c.rr_nxt[blockIdx.x] = frozen ? 0.f : dot;
}

// cg_res[r] = |r_iters| / |b|, 0 for a frozen row (its partials of r.r are 0) and for b = 0
__global__ __launch_bounds__(KS_THREADS) void k_sn_residual(const float* rr, const float* bb, float* cg_res, int rows, int tiles) {
  const int r = blockIdx.x * KS_THREADS + threadIdx.x;
  if (r >= rows) return;
  const double a = sn_row_sum(rr, r, tiles), b = sn_row_sum(bb, r, tiles);
  cg_res[r] = (a == 0.0 || b == 0.0) ? 0.f : (float)sqrt(a / b);
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------------
struct sn_grid {
  int logS, logL;
  dim3 rows, cols;
  size_t lds;
};

// the sizes every entry shares -> the launch geometry
static int sn_sizes(const char* who, int rows, int coils, int map_rows, int S, sn_grid& g) {
  g.logS = ks_log2(S);
  MUD_REQUIRE(g.logS > 0, "%s: S must be a power of two in [%d, %d], got %d", who, KS_MIN_S, KS_MAX_S, S);
  MUD_REQUIRE(rows > 0 && (int64_t)rows * S * S < (1ll << 31), "%s: rows must be > 0 with rows * S * S < 2^31, got %d", who, rows);
  MUD_REQUIRE(coils >= 1 && coils <= SN_MAX_COILS, "%s: coils must be in [1, %d], got %d", who, SN_MAX_COILS, coils);
  MUD_REQUIRE(map_rows == 1 || map_rows == rows, "%s: map_rows must be 1 or rows (%d), got %d", who, rows, map_rows);
  MUD_REQUIRE((int64_t)rows * coils * S * S < (1ll << 31), "%s: rows * coils * S * S must be < 2^31, got %d * %d * %d * %d", who, rows, coils, S, S);
  g.logL = ks_log_lines(S);
  g.rows = dim3((unsigned)(((int64_t)rows << g.logS) >> g.logL));
  g.cols = dim3((unsigned)((int64_t)rows * coils * (S >> g.logL)));
  g.lds = ks_lds_bytes(S);
  return MUD_OK;
}

static inline int64_t sn_tiles(int S) { return S >> ks_log_lines(S); }

extern "C" int64_t mud_sense_ws_floats(int rows, int coils, int S) {
  if (rows < 1 || coils < 1 || coils > SN_MAX_COILS || ks_log2(S) < 0) return -1;
  const int64_t px = (int64_t)rows * S * S;
  return 2 * px * coils + 4 * px + 4 * rows * sn_tiles(S);
}

static inline bool sn_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

extern "C" int mud_sense_constrain(const float* x_new, const float* ahy, const uint8_t* mask, int mask_rows, const float* maps, int map_rows, int coils,
                                   float lambda, int iters, const float* noise, const int64_t* keys, uint64_t seed, int step, int kind,
                                   const int64_t* t, int toff, const float* a_tab, const float* s_tab, int ntab, int clean, float* out,
                                   float* cg_res, float* work, int rows, int S, void* stream) {
  const char* who = "mud_sense_constrain";
  sn_con c = {};
  c.x_new = x_new, c.ahy = ahy, c.maps = reinterpret_cast<const float2*>(maps), c.map_rows = map_rows, c.coils = coils, c.lambda = lambda;
  c.d = {noise, keys, seed, 0, t, toff, a_tab, s_tab, ntab, clean};
  c.out = out;
  sn_grid g;
  MUD_TRY(sn_sizes(who, rows, coils, map_rows, S, g));
  MUD_REQUIRE(mask_rows == 1 || mask_rows == rows, "%s: mask_rows must be 1 or rows (%d), got %d", who, rows, mask_rows);
  MUD_REQUIRE(iters >= 1 && iters <= SN_MAX_ITERS, "%s: iters must be in [1, %d], got %d", who, SN_MAX_ITERS, iters);
  MUD_REQUIRE(lambda >= 0.f && lambda - lambda == 0.f, "%s: lambda must be finite and >= 0, got %g", who, (double)lambda);
  MUD_TRY(keyed_level_word2(who, ntab, kind, step, c.d.word2));
  MUD_REQUIRE(x_new && ahy && mask && maps && out && cg_res && work, "%s: null pointer (x_new, ahy, mask, maps, out, cg_res, work)", who);
  MUD_TRY(keyed_level_operands(who, true, c.d));
  MUD_REQUIRE(mud_aligned16(x_new) && mud_aligned16(out) && mud_aligned16(ahy) && mud_aligned16(work) && (!noise || mud_aligned16(noise)) &&
                  ((uintptr_t)maps & 7u) == 0,
              "%s: x_new, ahy, out, noise and work must be 16-byte aligned, maps 8-byte", who);
  const int64_t px = (int64_t)rows * S * S, tiles = sn_tiles(S), wbytes = mud_sense_ws_floats(rows, coils, S) * 4;
  MUD_REQUIRE(!sn_overlap(work, wbytes, x_new, px * 4) && !sn_overlap(work, wbytes, out, px * 4) && !sn_overlap(work, wbytes, ahy, px * 4) &&
                  !sn_overlap(work, wbytes, noise, px * 4) && !sn_overlap(work, wbytes, cg_res, (int64_t)rows * 4) &&
                  !sn_overlap(work, wbytes, maps, (int64_t)map_rows * coils * S * S * 8) &&
                  !sn_overlap(work, wbytes, mask, (int64_t)mask_rows * S * S),
              "%s: work must be a buffer of its own", who);
  float2* w = reinterpret_cast<float2*>(work);
  float* v = work + 2 * px * coils;
  c.r = v, c.p = v + px, c.q = v + 2 * px, c.e = v + 3 * px;
  float* part = v + 4 * px;
  float* rr[2] = {part + rows * tiles, part + 2 * rows * tiles};
  c.bb = part, c.pq = part + 3 * rows * tiles;
  hipStream_t st = (hipStream_t)stream;
  const dim3 th(KS_THREADS);
  // b = N (x_new - s eta) - a A^H y -> r, |b|^2
  c.rr_cur = rr[0], c.rr_nxt = rr[1];
  hipLaunchKernelGGL(k_sn_rows_fwd<SN_FWD_FIRST>, g.rows, th, g.lds, st, (const float*)nullptr, w, c, g.logS, g.logL);
  MUD_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(k_sn_cols<SN_COL_NORMAL>, g.cols, th, g.lds, st, w, mask, mask_rows, coils, g.logS, g.logL);
  MUD_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(k_sn_rows_inv<SN_INV_FIRST>, g.rows, th, g.lds, st, (const float2*)w, c, g.logS, g.logL);
  MUD_CHECK_LAUNCH(who);
  for (int k = 0; k < iters; ++k) {
    c.rr_cur = rr[k & 1], c.rr_nxt = rr[(k & 1) ^ 1];
    if (k == 0)
      hipLaunchKernelGGL(k_sn_rows_fwd<SN_FWD_P_INIT>, g.rows, th, g.lds, st, (const float*)nullptr, w, c, g.logS, g.logL);
    else
      hipLaunchKernelGGL(k_sn_rows_fwd<SN_FWD_P_NEXT>, g.rows, th, g.lds, st, (const float*)nullptr, w, c, g.logS, g.logL);
    MUD_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(k_sn_cols<SN_COL_NORMAL>, g.cols, th, g.lds, st, w, mask, mask_rows, coils, g.logS, g.logL);
    MUD_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(k_sn_rows_inv<SN_INV_CG>, g.rows, th, g.lds, st, (const float2*)w, c, g.logS, g.logL);
    MUD_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(k_sn_update, g.rows, th, 0, st, c, g.logS, g.logL, k == 0, k == iters - 1);
    MUD_CHECK_LAUNCH(who);
  }
  hipLaunchKernelGGL(k_sn_residual, dim3((unsigned)mud_cdiv(rows, KS_THREADS)), th, 0, st, (const float*)rr[iters & 1], (const float*)c.bb, cg_res, rows,
                     (int)tiles);
  MUD_CHECK_LAUNCH(who);
  return MUD_OK;
}

extern "C" int mud_sense_measure(const float* x, const float* maps, int map_rows, int coils, const uint8_t* mask, int mask_rows, float* y, int rows,
                                 int S, void* stream) {
  const char* who = "mud_sense_measure";
  sn_con c = {};
  c.maps = reinterpret_cast<const float2*>(maps), c.map_rows = map_rows, c.coils = coils;
  sn_grid g;
  MUD_TRY(sn_sizes(who, rows, coils, map_rows, S, g));
  MUD_REQUIRE(mask_rows == 1 || mask_rows == rows, "%s: mask_rows must be 1 or rows (%d), got %d", who, rows, mask_rows);
  MUD_REQUIRE(x && maps && mask && y, "%s: null pointer (x, maps, mask, y)", who);
  MUD_REQUIRE(mud_aligned16(x) && (((uintptr_t)maps | (uintptr_t)y) & 7u) == 0, "%s: x must be 16-byte aligned, maps and y 8-byte", who);
  MUD_REQUIRE(!sn_overlap(y, (int64_t)rows * coils * S * S * 8, x, (int64_t)rows * S * S * 4), "%s: y must not overlap x", who);
  hipStream_t st = (hipStream_t)stream;
  float2* w = reinterpret_cast<float2*>(y);
  hipLaunchKernelGGL(k_sn_rows_fwd<SN_FWD_PLAIN>, g.rows, dim3(KS_THREADS), g.lds, st, x, w, c, g.logS, g.logL);
  MUD_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(k_sn_cols<SN_COL_MEASURE>, g.cols, dim3(KS_THREADS), g.lds, st, w, mask, mask_rows, coils, g.logS, g.logL);
  MUD_CHECK_LAUNCH(who);
  return MUD_OK;
}

extern "C" int mud_sense_adjoint(float* y, const float* maps, int map_rows, int coils, float* out, int rows, int S, void* stream) {
  const char* who = "mud_sense_adjoint";
  sn_con c = {};
  c.maps = reinterpret_cast<const float2*>(maps), c.map_rows = map_rows, c.coils = coils, c.out = out;
  sn_grid g;
  MUD_TRY(sn_sizes(who, rows, coils, map_rows, S, g));
  MUD_REQUIRE(y && maps && out, "%s: null pointer (y, maps, out)", who);
  MUD_REQUIRE(mud_aligned16(out) && (((uintptr_t)maps | (uintptr_t)y) & 7u) == 0, "%s: out must be 16-byte aligned, maps and y 8-byte", who);
  MUD_REQUIRE(!sn_overlap(y, (int64_t)rows * coils * S * S * 8, out, (int64_t)rows * S * S * 4), "%s: out must not overlap y", who);
  hipStream_t st = (hipStream_t)stream;
  float2* w = reinterpret_cast<float2*>(y);
  hipLaunchKernelGGL((k_ks_cols<false, ks_level_own>), g.cols, dim3(KS_THREADS), g.lds, st, w, (const float2*)nullptr, (const uint8_t*)nullptr, 1,
                     (const int64_t*)nullptr, 0, (const float*)nullptr, 1, 1, g.logS, g.logL, 1, ks_level_own{});
  MUD_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(k_sn_rows_inv<SN_INV_ADJOINT>, g.rows, dim3(KS_THREADS), g.lds, st, (const float2*)w, c, g.logS, g.logL);
  MUD_CHECK_LAUNCH(who);
  return MUD_OK;
}
