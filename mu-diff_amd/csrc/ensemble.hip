// N-sample ensemble inference (include/mudiff_hip.h: mud_randn_keyed, mud_ensemble_stats, mud_ensemble_quantiles).
//
// The sampler is stochastic: x_init, every step's latent z and every step's posterior noise are Gaussian draws.  Sampling a slice N
// times and reporting the per-pixel mean and spread shows where a synthesis is unsure of itself.  Two kernels serve it:
//  - keyed draws: every Gaussian is a pure function of (seed, slice, sample, step, kind, element) through counter-based
//    Philox4x64-10 (Random123; the algorithm and word order of numpy.random.Philox), so an ensemble does not depend on batch size,
//    chunking or rank count, and nothing is pre-drawn;
//  - statistics: per pixel, the fp64 mean and unbiased standard deviation over the N samples, summed in sample order with no
//    atomics and no contraction: a fixed function of the samples;
//  - order statistics: per pixel, up to 8 quantiles of the N samples (the median, an interval's bounds) from a sorting network in
//    registers: the same one read of the samples, a fixed function of them as well.
// DESIGN.md section 5.7 has the definitions and the order arguments.
#include "keyed_rows.h"        // the quad mapping and store, and keyed_normal.h: es_philox, es_box_muller, es_block_normals

#define ES_THREADS 256

// one thread = one Philox block = one quad of one row.  VEC: row_len % 4 == 0 and out 16-byte aligned: every block is whole and aligned
template <bool VEC>
__global__ __launch_bounds__(ES_THREADS) void k_randn_keyed(float* __restrict__ out, int rows, int64_t row_len, int64_t blocks_per_row,
                                                            const int64_t* __restrict__ keys, uint64_t seed, uint64_t word2) {
  row_quad q;
  if (!row_quad_of<VEC>((int64_t)blockIdx.x * ES_THREADS + threadIdx.x, rows, row_len, blocks_per_row, q)) return;
  quad_store<VEC>(out + q.base, es_block_normals((uint64_t)q.b, (uint64_t)keys[2 * q.r], (uint64_t)keys[2 * q.r + 1], seed, word2), q.n);
}

extern "C" int mud_randn_keyed(float* out, int rows, int64_t row_len, const int64_t* keys, uint64_t seed, int step, int kind, void* stream) {
  MUD_REQUIRE(rows >= 0 && row_len > 0, "mud_randn_keyed: bad sizes (rows %d, row_len %lld)", rows, (long long)row_len);
  MUD_REQUIRE((kind >= 0 && kind <= 2) || (kind >= 5 && kind <= 11),
              "mud_randn_keyed: kind must be 0 (x_init), 1 (z), 2 (posterior noise), 5 (k-space), 6 (thick slices), 7 (multislice), 8 (thick "
              "volume), 9 (low-resolution volume), 10 (multi-coil) or 11 (multi-coil measurement noise), got %d", kind);
  uint64_t word2;
  MUD_TRY(keyed_step_word2("mud_randn_keyed", step, kind, word2));
  MUD_REQUIRE(out && keys, "mud_randn_keyed: null pointer");
  if (rows == 0) return MUD_OK;
  const int64_t bpr = mud_cdiv(row_len, 4);
  const int64_t threads = (int64_t)rows * bpr;
  MUD_REQUIRE(mud_cdiv(threads, ES_THREADS) <= 0x7fffffff, "mud_randn_keyed: too many elements");
  vec_dispatch(row_len % 4 == 0 && mud_aligned16(out), [&](auto v) {
    hipLaunchKernelGGL(k_randn_keyed<VEC_OF(v)>, dim3((unsigned)mud_cdiv(threads, ES_THREADS)), dim3(ES_THREADS), 0, (hipStream_t)stream, out, rows,
                       row_len, bpr, keys, seed, word2);
  });
  MUD_CHECK_LAUNCH("mud_randn_keyed");
  return MUD_OK;
}

// ---- slice-coupled keyed draws (mudiff_hip.slice_coupling) --------------------------------------------------
// out[r, e] = fp32(sum_{j=-R..R} w_|j| * eta(seed, s + j, m, step, kind)[e]) with eta the fp32 value of k_randn_keyed for that key: the
// white noise of the slices around s, filtered along z.  With sum w^2 = 1 every row stays N(0, 1) per element, and two rows d slices apart
// correlate by sum_j w_j w_{j+d}.  s + j wraps modulo 2^64 (the Philox counter word), so the first slices of a volume see the same
// statistics as the others.  The half taps travel as a kernel argument: nothing is allocated and nothing read from the device but the keys.
#define ES_MAX_RADIUS MUD_COUPLING_MAX_RADIUS
struct es_taps {
  double w[ES_MAX_RADIUS + 1];
};

// the thread mapping and the store of k_randn_keyed; per tap one Philox block and its two Box-Muller pairs, the products and
// the sums in fp64 in tap order j = -R..R, each rounded once (no contraction), the result rounded to fp32 once
template <bool VEC>
__global__ __launch_bounds__(ES_THREADS) void k_randn_keyed_coupled(float* __restrict__ out, int rows, int64_t row_len, int64_t blocks_per_row,
                                                                    const int64_t* __restrict__ keys, uint64_t seed, uint64_t word2, es_taps taps,
                                                                    int radius) {
#pragma clang fp contract(off)
  row_quad q;
  if (!row_quad_of<VEC>((int64_t)blockIdx.x * ES_THREADS + threadIdx.x, rows, row_len, blocks_per_row, q)) return;
  const uint64_t slice = (uint64_t)keys[2 * q.r], sample = (uint64_t)keys[2 * q.r + 1];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = -radius; j <= radius; ++j) {                // uniform over the launch
    const double w = taps.w[j < 0 ? -j : j];
    uint64_t c0 = (uint64_t)q.b, c1 = slice + (uint64_t)(int64_t)j, c2 = (sample << 32) | word2, c3 = 0;
    es_philox(c0, c1, c2, c3, seed, ES_KEY_HI);
    float e0, e1, e2, e3;
    es_box_muller(c0, c1, e0, e1);
    es_box_muller(c2, c3, e2, e3);
    acc[0] = acc[0] + w * (double)e0;
    acc[1] = acc[1] + w * (double)e1;
    acc[2] = acc[2] + w * (double)e2;
    acc[3] = acc[3] + w * (double)e3;
  }
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (float)acc[e];
  quad_store<VEC>(out + q.base, v, q.n);
}

extern "C" int mud_randn_keyed_coupled(float* out, int rows, int64_t row_len, const int64_t* keys, uint64_t seed, int step, int kind,
                                       const double* half_taps, int radius, void* stream) {
  MUD_REQUIRE(rows >= 0 && row_len > 0, "mud_randn_keyed_coupled: bad sizes (rows %d, row_len %lld)", rows, (long long)row_len);
  MUD_REQUIRE(kind >= 0 && kind <= 2, "mud_randn_keyed_coupled: kind must be 0 (x_init), 1 (z) or 2 (posterior noise), got %d", kind);
  uint64_t word2;
  MUD_TRY(keyed_step_word2("mud_randn_keyed_coupled", step, kind, word2));
  MUD_REQUIRE(radius >= 0 && radius <= ES_MAX_RADIUS, "mud_randn_keyed_coupled: radius must be in [0, %d], got %d", ES_MAX_RADIUS, radius);
  MUD_REQUIRE(out && keys && half_taps, "mud_randn_keyed_coupled: null pointer");
  es_taps taps;
  for (int j = 0; j <= ES_MAX_RADIUS; ++j) {
    taps.w[j] = j <= radius ? half_taps[j] : 0.0;
    MUD_REQUIRE(taps.w[j] - taps.w[j] == 0.0, "mud_randn_keyed_coupled: tap %d is not finite", j);
  }
  if (rows == 0) return MUD_OK;
  const int64_t bpr = mud_cdiv(row_len, 4);
  const int64_t threads = (int64_t)rows * bpr;
  MUD_REQUIRE(mud_cdiv(threads, ES_THREADS) <= 0x7fffffff, "mud_randn_keyed_coupled: too many elements");
  vec_dispatch(row_len % 4 == 0 && mud_aligned16(out), [&](auto v) {
    hipLaunchKernelGGL(k_randn_keyed_coupled<VEC_OF(v)>, dim3((unsigned)mud_cdiv(threads, ES_THREADS)), dim3(ES_THREADS), 0, (hipStream_t)stream, out,
                       rows, row_len, bpr, keys, seed, word2, taps, radius);
  });
  MUD_CHECK_LAUNCH("mud_randn_keyed_coupled");
  return MUD_OK;
}

// ---- per-pixel ensemble statistics --------------------------------------------------------------------------------------------------
// y = clamp(x*scale + shift, lo, hi) with the fp32 steps of mud_affine_clamp, each rounded once (no contraction); unlike fminf / fmaxf
// alone, a NaN stays NaN (np.clip semantics) so that it reaches both outputs
__device__ __forceinline__ float es_premap(float x, float scale, float shift, float lo, float hi) {
#pragma clang fp contract(off)
  const float t = x * scale + shift;
  return t != t ? t : fminf(fmaxf(t, lo), hi);
}

// m = (sum_j y_j) / N and v = sum_j (y_j - m)^2 / (N - 1), fp64 in sample order j = 0..N-1.  Up to ES_CAP samples stay in registers
// (one read of the samples); more are read a second time for the deviations.
#define ES_CAP 16
template <int W>
__device__ __forceinline__ void es_load(const float* __restrict__ p, float (&x)[W]) {
  if constexpr (W == 4) {           // 16-byte aligned (k_ensemble_stats4): one dwordx4 load
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int w = 0; w < 4; ++w) x[w] = v[w];
  } else {
#pragma unroll
    for (int w = 0; w < W; ++w) x[w] = p[w];
  }
}

template <int W>
__device__ __forceinline__ void es_stats(const float* __restrict__ src, int N, int64_t hw, float scale, float shift, float lo, float hi,
                                         double (&m)[W], double (&v)[W]) {
#pragma clang fp contract(off)
  float y[ES_CAP][W];
  double s[W];
#pragma unroll
  for (int w = 0; w < W; ++w) s[w] = 0.0;
#pragma unroll
  for (int j = 0; j < ES_CAP; ++j) {
    if (j < N) {
      float x[W];
      es_load<W>(src + (int64_t)j * hw, x);
#pragma unroll
      for (int w = 0; w < W; ++w) {
        y[j][w] = es_premap(x[w], scale, shift, lo, hi);
        s[w] += (double)y[j][w];
      }
    }
  }
  for (int j = ES_CAP; j < N; ++j) {
    float x[W];
    es_load<W>(src + (int64_t)j * hw, x);
#pragma unroll
    for (int w = 0; w < W; ++w) s[w] += (double)es_premap(x[w], scale, shift, lo, hi);
  }
#pragma unroll
  for (int w = 0; w < W; ++w) {
    m[w] = s[w] / (double)N;
    v[w] = 0.0;
  }
#pragma unroll
  for (int j = 0; j < ES_CAP; ++j) {
    if (j < N) {
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const double d = (double)y[j][w] - m[w];
        v[w] += d * d;
      }
    }
  }
  for (int j = ES_CAP; j < N; ++j) {
    float x[W];
    es_load<W>(src + (int64_t)j * hw, x);
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const double d = (double)es_premap(x[w], scale, shift, lo, hi) - m[w];
      v[w] += d * d;
    }
  }
#pragma unroll
  for (int w = 0; w < W; ++w) v[w] = v[w] / (double)(N - 1);
}

// one thread = 4 consecutive pixels of one slice (vec: hw % 4 == 0 and every pointer 16-byte aligned), else one pixel
__global__ __launch_bounds__(ES_THREADS) void k_ensemble_stats4(const float* __restrict__ x, int n, int N, int64_t hw, float scale, float shift,
                                                                float lo, float hi, float* __restrict__ mean, float* __restrict__ std) {
  const int64_t q = hw / 4;
  const int64_t t = (int64_t)blockIdx.x * ES_THREADS + threadIdx.x;
  if (t >= (int64_t)n * q) return;
  const int64_t i = t / q, p = 4 * (t - i * q);
  const float* src = x + (int64_t)i * N * hw + p;
  double m[4], v[4];
  es_stats<4>(src, N, hw, scale, shift, lo, hi, m, v);
  f32x4 om, os;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    om[w] = (float)m[w];
    os[w] = (float)sqrt(v[w]);
  }
  *reinterpret_cast<f32x4*>(mean + i * hw + p) = om;
  *reinterpret_cast<f32x4*>(std + i * hw + p) = os;
}

__global__ __launch_bounds__(ES_THREADS) void k_ensemble_stats1(const float* __restrict__ x, int n, int N, int64_t hw, float scale, float shift,
                                                                float lo, float hi, float* __restrict__ mean, float* __restrict__ std) {
  const int64_t t = (int64_t)blockIdx.x * ES_THREADS + threadIdx.x;
  if (t >= (int64_t)n * hw) return;
  const int64_t i = t / hw, p = t - i * hw;
  double m[1], v[1];
  es_stats<1>(x + (int64_t)i * N * hw + p, N, hw, scale, shift, lo, hi, m, v);
  mean[i * hw + p] = (float)m[0];
  std[i * hw + p] = (float)sqrt(v[0]);
}

extern "C" int mud_ensemble_stats(const float* samples, int n, int N, int64_t hw, float scale, float shift, float lo, float hi, float* mean,
                                  float* std, void* stream) {
  MUD_REQUIRE(n >= 0 && hw > 0, "mud_ensemble_stats: bad sizes (n %d, hw %lld)", n, (long long)hw);
  MUD_REQUIRE(N >= 2, "mud_ensemble_stats: N must be >= 2 (the spread needs two samples), got %d", N);
  MUD_REQUIRE(samples && mean && std, "mud_ensemble_stats: null pointer");
  if (n == 0) return MUD_OK;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = hw % 4 == 0 && mud_aligned16(samples) && mud_aligned16(mean) && mud_aligned16(std);
  const int64_t threads = vec ? (int64_t)n * (hw / 4) : (int64_t)n * hw;
  MUD_REQUIRE(mud_cdiv(threads, ES_THREADS) <= 0x7fffffff, "mud_ensemble_stats: too many pixels");
  const dim3 grid((unsigned)mud_cdiv(threads, ES_THREADS));
  if (vec)
    hipLaunchKernelGGL(k_ensemble_stats4, grid, dim3(ES_THREADS), 0, s, samples, n, N, hw, scale, shift, lo, hi, mean, std);
  else
    hipLaunchKernelGGL(k_ensemble_stats1, grid, dim3(ES_THREADS), 0, s, samples, n, N, hw, scale, shift, lo, hi, mean, std);
  MUD_CHECK_LAUNCH("mud_ensemble_stats");
  return MUD_OK;
}

// ---- per-pixel quantiles --------------------------------------------------------------------------------------------------------------
// With y_(0) <= ... <= y_(N-1) the pre-mapped (es_premap) samples of a pixel in ascending order and q a fraction in [0, 1]:
//   h = (N - 1) * q,  i = min(floor(h), N - 2),  g = h - i,  out = fp32(y_(i) + g * (y_(i+1) - y_(i))),
// everything from h on in fp64, each operation rounded once (no contraction).  A pixel with a NaN sample gives NaN for every q
// (np.quantile's rule): v_min_f32 / v_max_f32 drop a NaN, so it is replaced by +inf for the sort and remembered beside it.
// One thread sorts the samples of W pixels in registers: N is padded to NP, a power of two, with +inf (which sorts behind every sample,
// ties included: only y_(0..N-1) are ever read), and a bitonic network of NP/2 * log2(NP) * (log2(NP) + 1) / 2 min / max pairs, fully
// unrolled, does the rest.  Every index of y[][] is a compile-time constant, so the array lives in VGPRs; the order statistic of a
// fraction is picked by NP selects on the (launch-uniform) index.  The fractions travel as a kernel argument.
#define EQ_MAX_K MUD_ENSEMBLE_MAX_QUANTILES
#define EQ_MAX_N MUD_ENSEMBLE_QUANTILES_MAX_N
struct eq_fracs {
  double q[EQ_MAX_K];
};

template <int NP, int W>
__device__ __forceinline__ void eq_sort(float (&y)[NP][W]) {
#pragma unroll
  for (int lk = 1; (1 << lk) <= NP; ++lk) {               // merge sorted runs of 2^(lk-1) into runs of 2^lk, alternately up and down
#pragma unroll
    for (int lj = lk - 1; lj >= 0; --lj) {
#pragma unroll
      for (int a = 0; a < NP; ++a) {
        const int b = a ^ (1 << lj);
        if (b > a) {
          const bool up = (a & (1 << lk)) == 0;
#pragma unroll
          for (int w = 0; w < W; ++w) {
            const float mn = fminf(y[a][w], y[b][w]), mx = fmaxf(y[a][w], y[b][w]);
            y[a][w] = up ? mn : mx;
            y[b][w] = up ? mx : mn;
          }
        }
      }
    }
  }
}

// one thread = W consecutive pixels of one slice; W == 4 under k_ensemble_stats4's condition (hw % 4 == 0, every pointer 16-byte aligned)
template <int NP, int W>
__global__ __launch_bounds__(ES_THREADS) void k_ensemble_quantiles(const float* __restrict__ x, int n, int N, int64_t hw, float scale, float shift,
                                                                   float lo, float hi, eq_fracs fr, int K, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t per = hw / W;
  const int64_t t = (int64_t)blockIdx.x * ES_THREADS + threadIdx.x;
  if (t >= (int64_t)n * per) return;
  const int64_t i = t / per, p = W * (t - i * per);
  const float* src = x + (int64_t)i * N * hw + p;
  const float inf = __builtin_inff();
  float y[NP][W];
  bool bad[W];
#pragma unroll
  for (int w = 0; w < W; ++w) bad[w] = false;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    if (j < N) {                                            // uniform over the launch
      float v[W];
      es_load<W>(src + (int64_t)j * hw, v);
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const float m = es_premap(v[w], scale, shift, lo, hi);
        bad[w] = bad[w] || m != m;
        y[j][w] = m != m ? inf : m;
      }
    } else {
#pragma unroll
      for (int w = 0; w < W; ++w) y[j][w] = inf;
    }
  }
  eq_sort<NP, W>(y);
  float* dst = out + i * hw + p;
#pragma unroll
  for (int k = 0; k < EQ_MAX_K; ++k) {
    if (k < K) {                                            // uniform over the launch, like idx and g
      const double h = (double)(N - 1) * fr.q[k];
      int idx = (int)floor(h);
      idx = idx > N - 2 ? N - 2 : idx;
      const double g = h - (double)idx;
      float r[W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        float a = y[0][w], b = y[1][w];
#pragma unroll
        for (int j = 1; j < NP - 1; ++j) {
          a = j == idx ? y[j][w] : a;
          b = j == idx ? y[j + 1][w] : b;
        }
        const double d = (double)b - (double)a;
        const double e = g * d;
        r[w] = bad[w] ? __builtin_nanf("") : (float)((double)a + e);
      }
      float* o = dst + (int64_t)k * n * hw;
      if constexpr (W == 4) {
        f32x4 ov;
#pragma unroll
        for (int w = 0; w < 4; ++w) ov[w] = r[w];
        *reinterpret_cast<f32x4*>(o) = ov;
      } else {
#pragma unroll
        for (int w = 0; w < W; ++w) o[w] = r[w];
      }
    }
  }
}

template <int NP, int W>
static void eq_launch(dim3 grid, hipStream_t s, const float* samples, int n, int N, int64_t hw, float scale, float shift, float lo, float hi,
                      const eq_fracs& fr, int K, float* out) {
  hipLaunchKernelGGL((k_ensemble_quantiles<NP, W>), grid, dim3(ES_THREADS), 0, s, samples, n, N, hw, scale, shift, lo, hi, fr, K, out);
}

// NP <= EQ_VEC_NP sorts 4 pixels per thread on the aligned path (NP = 32: 196 VGPRs, 2 waves per SIMD); the 256 values of NP = 64 do
// not fit the register file without scratch, so that size sorts one pixel per thread on both paths (scripts/kernel_resources.py;
// DESIGN.md section 5.24)
#define EQ_VEC_NP 32
template <int NP>
static void eq_dispatch(bool vec, int64_t blocks1, int64_t blocks4, hipStream_t s, const float* samples, int n, int N, int64_t hw, float scale,
                        float shift, float lo, float hi, const eq_fracs& fr, int K, float* out) {
  if constexpr (NP <= EQ_VEC_NP) {
    if (vec) return eq_launch<NP, 4>(dim3((unsigned)blocks4), s, samples, n, N, hw, scale, shift, lo, hi, fr, K, out);
  }
  eq_launch<NP, 1>(dim3((unsigned)blocks1), s, samples, n, N, hw, scale, shift, lo, hi, fr, K, out);
}

extern "C" int mud_ensemble_quantiles(const float* samples, int n, int N, int64_t hw, float scale, float shift, float lo, float hi,
                                      const double* q, int K, float* out, void* stream) {
  MUD_REQUIRE(n >= 0 && hw > 0, "mud_ensemble_quantiles: bad sizes (n %d, hw %lld)", n, (long long)hw);
  MUD_REQUIRE(N >= 2 && N <= EQ_MAX_N, "mud_ensemble_quantiles: N must be in [2, %d], got %d", EQ_MAX_N, N);
  MUD_REQUIRE(K >= 1 && K <= EQ_MAX_K, "mud_ensemble_quantiles: 1 to %d quantiles, got %d", EQ_MAX_K, K);
  MUD_REQUIRE(samples && q && out, "mud_ensemble_quantiles: null pointer");
  eq_fracs fr;
  for (int k = 0; k < EQ_MAX_K; ++k) {
    fr.q[k] = k < K ? q[k] : 0.0;
    MUD_REQUIRE(fr.q[k] >= 0.0 && fr.q[k] <= 1.0, "mud_ensemble_quantiles: quantile %d (%g) is not in [0, 1]", k, fr.q[k]);      // (a NaN fails it)
  }
  if (n == 0) return MUD_OK;
  const bool vec = hw % 4 == 0 && mud_aligned16(samples) && mud_aligned16(out);
  const int64_t blocks1 = mud_cdiv((int64_t)n * hw, ES_THREADS), blocks4 = mud_cdiv((int64_t)n * (hw / 4), ES_THREADS);
  MUD_REQUIRE(blocks1 <= 0x7fffffff, "mud_ensemble_quantiles: too many pixels");
  hipStream_t s = (hipStream_t)stream;
#define EQ_CASE(NP) eq_dispatch<NP>(vec, blocks1, blocks4, s, samples, n, N, hw, scale, shift, lo, hi, fr, K, out)
  if (N <= 2) EQ_CASE(2);
  else if (N <= 4) EQ_CASE(4);
  else if (N <= 8) EQ_CASE(8);
  else if (N <= 16) EQ_CASE(16);
  else if (N <= 32) EQ_CASE(32);
  else EQ_CASE(64);
#undef EQ_CASE
  MUD_CHECK_LAUNCH("mud_ensemble_quantiles");
  return MUD_OK;
}
