// Sampling a target acquired as accelerated thick slices (include/mudiff_hip.h: mud_slab_kspace_constrain; mudiff_hip.multislice,
// DESIGN.md section 5.28).  A slab is a weighted average of L thin slices (slab.hip) whose in-plane Fourier coefficients were measured
// on a mask (kspace.hip): A = M F (w^T (x) I), A A^H = (sum w^2) M, and the data-consistency step is an exact projection,
//   d = sum_l w_l (x_l - s eta_l),  R = M ? F(d) - a y : 0,  c = Re F^H R,  x_l <- x_l - g_l c,  g_l = w_l / sum_m w_m^2,
// in three launches per table chunk: rows forward (the members' sum fused into the load), kspace_lines.h's column pass with the level of
// the group's first member, rows inverse (the members' correction fused into the store).  The sum over a group's members runs in the
// table's order whatever the rows' positions; a workgroup owns whole lines of one group's image and a thread the same quad of every
// member from load to store, so in place is allowed; no atomics, and a group's result is a function of its own rows, table and keys.
#include "keyed_rows.h"
#include "kspace_lines.h"
#include "slab_tables.h"

#pragma clang fp contract(off)   // s * eta, x - ., w * ., acc + ., g * re, x - c: each rounded once, as tests/multislice_ref.py states them

// ... or, for the column pass on a group's image, the level of the group's first member (slab.hip's rule)
struct sk_level_first {
  int row[SL_GROUPS];
  __device__ __forceinline__ int64_t operator()(int64_t q) const { return row[q]; }
};

// Lines per workgroup of the row passes: ks_log_lines(S), cut until a thread owns one quad of one line (S / 4 quads a line, 256 threads:
// 16 lines up to S = 64, then 8, 4, 2).  A thread walks every member of its quad, up to 16 draws in a row at a noise level, so the work is
// spread over four times the workgroups kspace.hip's row pass would start at S = 256; a line's transform does not depend on its tile.
static inline int sk_log_lines(int S) {
  int l = ks_log_lines(S);
  while (l > 0 && ((1 << l) * (S >> 2)) > KS_THREADS) --l;
  return l;
}

// Row pass: workgroup (b, q) owns the lines b * L .. b * L + L - 1 of the image of group q of this launch, `data` = work at the launch's
// first group.  A thread owns one quad of one line, which is Philox block (line << (logS - 2)) + quad of every member row, the block
// mud_kspace_constrain draws for that element.
//  FWD: acc = sum over the members, table order, of w * (x_new - s * eta) (clean: w * x_new) -> (acc, 0) -> forward DIF -> data;
// !FWD: data -> inverse DIT -> per member, table order, out = x_new - g * Re(.) (out may be x_new: read, then written, by one thread).
template <bool FWD>
__global__ __launch_bounds__(KS_THREADS) void k_sk_rows(const float* x_new, float2* data, sl_tables tab, keyed_level lv, float* out, int logS, int logL) {
  extern __shared__ float2 ks_lds[];
  const int S = 1 << logS, P = S + 1, L = 1 << logL;
  float2* x = ks_lds;
  float2* tw = ks_lds + L * P;
  const int q = blockIdx.y, u0 = (int)blockIdx.x << logL;
  const int s0 = tab.start[q], s1 = tab.start[q + 1];
  float2* image = data + ((int64_t)q << (2 * logS));
  ks_twiddles(tw, S);
  if constexpr (FWD) {
    float sg = 0.f;
    if (!lv.clean) sg = lv.st[mud_level_index(lv.t, tab.member[s0], lv.toff, lv.ntab)];      // the level of the group's first member
    for (int i = threadIdx.x; i < L * (S >> 2); i += KS_THREADS) {
      const int l = i >> (logS - 2), c4 = i & ((S >> 2) - 1);
      const int64_t u = u0 + l;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int s = s0; s < s1; ++s) {                     // table order
        const int64_t r = tab.member[s];
        const int64_t g = (((r << logS) + u) << logS) + 4 * c4;
        f32x4 d = quad_load<true>(x_new + g, 4);
        if (!lv.clean) {
          const f32x4 eta = quad_eta<true>(lv, r, (uint64_t)((u << (logS - 2)) + c4), g, 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float p = sg * eta[e];
            d[e] = d[e] - p;
          }
        }
        const float w = tab.w[s];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = w * d[e];
          acc[e] = acc[e] + p;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) x[l * P + 4 * c4 + e] = make_float2(acc[e], 0.f);
    }
    ks_lines_dif(x, P, logL, logS, tw, false);
    for (int i = threadIdx.x; i < L * S; i += KS_THREADS) {
      const int l = i >> logS, v = i & (S - 1);
      image[((int64_t)(u0 + l) << logS) + v] = x[l * P + ks_bitrev(v, logS)];
    }
  } else {
    for (int i = threadIdx.x; i < L * S; i += KS_THREADS) {
      const int l = i >> logS, v = i & (S - 1);
      x[l * P + ks_bitrev(v, logS)] = image[((int64_t)(u0 + l) << logS) + v];
    }
    ks_lines_dit(x, P, logL, logS, tw, true);
    for (int i = threadIdx.x; i < L * (S >> 2); i += KS_THREADS) {
      const int l = i >> (logS - 2), c4 = i & ((S >> 2) - 1);
      const int64_t u = u0 + l;
      f32x4 re;
#pragma unroll
      for (int e = 0; e < 4; ++e) re[e] = x[l * P + 4 * c4 + e].x;
      for (int s = s0; s < s1; ++s) {
        const int64_t g = ((((int64_t)tab.member[s] << logS) + u) << logS) + 4 * c4;
        f32x4 o = *reinterpret_cast<const f32x4*>(x_new + g);
        const float gain = tab.g[s];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float c = gain * re[e];
          const float v = o[e] - c;
          o[e] = c == 0.f ? o[e] : v;                     // a zero correction of either sign keeps x_new's bits, -0 included
        }
        *reinterpret_cast<f32x4*>(out + g) = o;
      }
    }
  }
}

extern "C" int mud_slab_kspace_constrain(const float* x_new, const float* y, const uint8_t* mask, int mask_rows, const int32_t* members,
                                         const float* weights, const float* gains, int groups, int L, const float* noise, const int64_t* keys,
                                         uint64_t seed, int step, int kind, const int64_t* t, int toff, const float* a_tab, const float* s_tab,
                                         int ntab, int clean, float* out, float* work, int rows, int S, void* stream) {
  const char* who = "mud_slab_kspace_constrain";
  keyed_level d = {noise, keys, seed, 0, t, toff, a_tab, s_tab, ntab, clean};
  const int logS = ks_log2(S);
  MUD_REQUIRE(logS > 0, "%s: S must be a power of two in [%d, %d], got %d", who, KS_MIN_S, KS_MAX_S, S);
  MUD_REQUIRE(rows > 0 && (int64_t)rows * S * S < (1ll << 31), "%s: rows must be > 0 with rows * S * S < 2^31, got %d", who, rows);
  MUD_REQUIRE(groups >= 0 && groups <= rows, "%s: groups must be in [0, rows = %d], got %d", who, rows, groups);
  MUD_REQUIRE(L >= 1 && L <= MUD_SLAB_MAX_MEMBERS, "%s: L must be in [1, %d], got %d", who, MUD_SLAB_MAX_MEMBERS, L);
  MUD_REQUIRE(groups == 0 || mask_rows == 1 || mask_rows == groups, "%s: mask_rows must be 1 or groups (%d), got %d", who, groups, mask_rows);
  MUD_TRY(keyed_level_word2(who, ntab, kind, step, d.word2));
  MUD_REQUIRE(x_new && out, "%s: null pointer (x_new, out)", who);
  MUD_REQUIRE(groups == 0 || (y && mask && work && members && weights && gains), "%s: null pointer (y, mask, work, members, weights, gains)", who);
  MUD_TRY(keyed_level_operands(who, groups != 0, d));
  MUD_REQUIRE(mud_aligned16(x_new) && mud_aligned16(out) && (!noise || mud_aligned16(noise)) && (((uintptr_t)y | (uintptr_t)work) & 7u) == 0,
              "%s: x_new, out and noise must be 16-byte aligned, y and work 8-byte", who);
  MUD_REQUIRE(groups == 0 || ((const void*)work != (const void*)x_new && (const void*)work != (const void*)out && (const void*)work != (const void*)y),
              "%s: work must be a buffer of its own", who);
  std::vector<sl_tables> launches;
  std::vector<int> first, count;
  std::vector<uint8_t> owner;
  MUD_TRY(sl_pack(who, members, weights, gains, groups, L, rows, launches, first, count, owner));
  const int64_t image = (int64_t)S * S;
  if (out != x_new) MUD_TRY(sl_copy_free_rows(who, x_new, out, owner, rows, image, stream));
  const int logL = ks_log_lines(S), logR = sk_log_lines(S);          // lines per workgroup: the column pass, the row passes
  const size_t lds = ks_lds_bytes(S), lds_rows = ks_lds_bytes_of(S, logR);
  hipStream_t st = (hipStream_t)stream;
  for (size_t i = 0; i < launches.size(); ++i) {
    const int n = count[i];
    const dim3 grid_rows((unsigned)(S >> logR), (unsigned)n), grid_cols((unsigned)(n * (S >> logL)));
    float2* w = reinterpret_cast<float2*>(work) + first[i] * image;
    sk_level_first level = {};
    for (int q = 0; q < n; ++q) level.row[q] = launches[i].member[launches[i].start[q]];
    hipLaunchKernelGGL(k_sk_rows<true>, grid_rows, dim3(KS_THREADS), lds_rows, st, x_new, w, launches[i], d, out, logS, logR);
    MUD_CHECK_LAUNCH(who);
    hipLaunchKernelGGL((k_ks_cols<true, sk_level_first>), grid_cols, dim3(KS_THREADS), lds, st, w, reinterpret_cast<const float2*>(y) + first[i] * image,
                       mask + (mask_rows == 1 ? 0 : first[i] * image), mask_rows, t, toff, a_tab, ntab, clean, logS, logL, 0, level);
    MUD_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(k_sk_rows<false>, grid_rows, dim3(KS_THREADS), lds_rows, st, x_new, w, launches[i], d, out, logS, logR);
    MUD_CHECK_LAUNCH(who);
  }
  return MUD_OK;
}
