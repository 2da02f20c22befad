// Sampling with a partly acquired target (include/mudiff_hip.h: mud_known_constrain, mud_known_coverage; mudiff_hip.known_region,
// DESIGN.md section 5.25).  Where the target contrast was acquired, the sampler re-imposes it after every reverse step at that step's
// noise level (RePaint, Lugmayr et al. 2022), so that the free region is sampled conditioned on the acquired voxels:
//  - constrain: out = mask ? q_sample(known) : x_new, one pass, the forward-diffusion noise drawn in the kernel with mud_randn_keyed's
//    keyed Philox draw (keyed_normal.h), so nothing is pre-drawn and a row's result depends on (seed, its key) alone;
//  - coverage: which voxels of a resampled known volume were interpolated from acquired voxels only.
// No LDS, no atomics: both are fixed functions of their inputs.
#include "keyed_rows.h"

#define KR_THREADS 256

// one thread = one quad (keyed_rows.h: row_quad_of).  out may alias x_new or known: a thread reads its 4 elements of each before it
// writes them, and no other thread touches them.  VEC: row_len % 4 == 0 and every pointer aligned for a 16-byte (mask: 4-byte) access.
template <bool VEC>
__global__ __launch_bounds__(KR_THREADS) void k_known_constrain(const float* x_new, const float* known, const uint8_t* __restrict__ mask, keyed_level d,
                                                                float* out, int rows, int64_t row_len, int64_t blocks_per_row) {
#pragma clang fp contract(off)   // a * known + sg * eta: mul, mul, add, each rounded once, in k_q_sample's order
  row_quad q;
  if (!row_quad_of<VEC>((int64_t)blockIdx.x * KR_THREADS + threadIdx.x, rows, row_len, blocks_per_row, q)) return;
  bool m[4] = {q.n > 0, q.n > 1, q.n > 2, q.n > 3};             // no mask: known everywhere
  f32x4 x = {0.f, 0.f, 0.f, 0.f};
  if (mask) {
    quad_load_mask<VEC>(mask + q.base, q.n, m);
    x = quad_load<VEC>(x_new + q.base, q.n);
  }
  f32x4 o = x;
  if (m[0] || m[1] || m[2] || m[3]) {            // a thread with nothing known skips the loads of `known` and the draw
    const f32x4 k = quad_load<VEC>(known + q.base, q.n);
    f32x4 ks = k;
    if (!d.clean) {
      const int64_t ti = mud_level_index(d.t, q.r, d.toff, d.ntab);
      const float a = d.at[ti], sg = d.st[ti];
      const f32x4 eta = quad_eta<VEC>(d, q.r, (uint64_t)q.b, q.base, q.n);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p0 = a * k[e], p1 = sg * eta[e];
        ks[e] = p0 + p1;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = m[e] ? ks[e] : x[e];     // a select: what `known` holds where the mask is 0 never reaches out
  }
  quad_store<VEC>(out + q.base, o, q.n);
}

extern "C" int mud_known_constrain(const float* x_new, const float* known, const uint8_t* mask, const float* noise, const int64_t* keys,
                                   uint64_t seed, int step, int kind, const int64_t* t, int toff, const float* a_tab, const float* s_tab,
                                   int ntab, int clean, float* out, int rows, int64_t row_len, void* stream) {
  keyed_level d = {noise, keys, seed, 0, t, toff, a_tab, s_tab, ntab, clean};
  MUD_REQUIRE(rows > 0 && row_len > 0, "mud_known_constrain: bad sizes (rows %d, row_len %lld)", rows, (long long)row_len);
  MUD_TRY(keyed_level_word2("mud_known_constrain", ntab, kind, step, d.word2));
  MUD_REQUIRE(known && out, "mud_known_constrain: null pointer (known, out)");
  MUD_REQUIRE(!mask || x_new, "mud_known_constrain: null pointer (x_new may be NULL only when mask is)");
  MUD_TRY(keyed_level_operands("mud_known_constrain", true, d));
  const int64_t bpr = mud_cdiv(row_len, 4);
  const int64_t threads = (int64_t)rows * bpr;
  MUD_REQUIRE(mud_cdiv(threads, KR_THREADS) <= 0x7fffffff, "mud_known_constrain: too many elements");
  const bool vec = row_len % 4 == 0 && mud_aligned16(known) && mud_aligned16(out) && (!mask || (mud_aligned16(x_new) && (((uintptr_t)mask) & 3u) == 0)) &&
                   (!noise || mud_aligned16(noise));
  vec_dispatch(vec, [&](auto v) {
    hipLaunchKernelGGL(k_known_constrain<VEC_OF(v)>, dim3((unsigned)mud_cdiv(threads, KR_THREADS)), dim3(KR_THREADS), 0, (hipStream_t)stream, x_new, known,
                       mask, d, out, rows, row_len, bpr);
  });
  MUD_CHECK_LAUNCH("mud_known_constrain");
  return MUD_OK;
}

// ---- coverage of a resampled volume ---------------------------------------------------------------------------------------------------
// p = m * (i, j, k, 1) in fp64 as mud_volume_regrid_cubic forms it: ((m0 * i + m1 * j) + m2 * k) + m3 per axis, every product and sum
// rounded separately.  One thread per destination voxel, x fastest.
struct kr_matrix {
  double m[12];
};

__global__ __launch_bounds__(KR_THREADS) void k_known_coverage(kr_matrix M, int SX, int SY, int SZ, int X, int Y, int64_t n, uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x;
  if (v >= n) return;
  const int64_t yz = v / X;
  const double i = (double)(v - yz * X), j = (double)(yz % Y), k = (double)(yz / Y);
  const double S[3] = {(double)(SX - 1), (double)(SY - 1), (double)(SZ - 1)};
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double p = ((M.m[4 * a] * i + M.m[4 * a + 1] * j) + M.m[4 * a + 2] * k) + M.m[4 * a + 3];
    in = in && p >= 0.0 && p <= S[a];           // (a NaN fails both)
  }
  out[v] = in ? 1 : 0;
}

extern "C" int mud_known_coverage(const double* m, int SX, int SY, int SZ, int X, int Y, int Z, uint8_t* out, void* stream) {
  MUD_REQUIRE(SX > 0 && SY > 0 && SZ > 0 && X > 0 && Y > 0 && Z > 0, "mud_known_coverage: bad sizes (source %d x %d x %d, destination %d x %d x %d)", SX,
              SY, SZ, X, Y, Z);
  MUD_REQUIRE((int64_t)X * Y * Z < (1ll << 31) && (int64_t)SX * SY * SZ < (1ll << 31), "mud_known_coverage: a volume needs X*Y*Z < 2^31");
  MUD_REQUIRE(m && out, "mud_known_coverage: null pointer");
  kr_matrix M;
  for (int q = 0; q < 12; ++q) {
    M.m[q] = m[q];
    MUD_REQUIRE(M.m[q] - M.m[q] == 0.0, "mud_known_coverage: matrix entry %d is not finite", q);
  }
  const int64_t n = (int64_t)X * Y * Z;
  hipLaunchKernelGGL(k_known_coverage, dim3((unsigned)mud_cdiv(n, KR_THREADS)), dim3(KR_THREADS), 0, (hipStream_t)stream, M, SX, SY, SZ, X, Y, n, out);
  MUD_CHECK_LAUNCH("mud_known_coverage");
  return MUD_OK;
}
