// Sampling a target acquired with thick slices (include/mudiff_hip.h: mud_slab_constrain, mud_slab_average; mudiff_hip.thick, DESIGN.md
// section 5.27).  A thick slice (a slab) is a weighted average of L thin slices, y = sum_l w_l k_l per pixel; slabs do not overlap, so
// A A^T is diagonal and the data-consistency step is an exact orthogonal projection along the profile:
//  - constrain: r = sum_l w_l (x_l - s eta_l) - a y, x_l <- x_l - g_l r for every member row l of a group, g_l = w_l / sum_m w_m^2;
//  - average:   avg = sum_l w_l x_l, the measurement of k and the residual's A x.
// This is the first constraint that couples the rows of a batch.  The sum over a group's members runs in the table's order whatever the
// rows' positions, one thread owns 4 consecutive elements of one group (all its members), and the draw is keyed (keyed_normal.h): a
// group's result is a function of its own rows, its table and its keys alone.  No LDS, no atomics, no contraction.
#include "keyed_rows.h"
#include "slab_tables.h"          // sl_tables, sl_pack, sl_copy_free_rows: shared with slab_kspace.hip

#define SL_THREADS 256
// grid (blocks over the row's quads, groups of this launch).  AVERAGE: out = avg [groups][row_len], nothing else is written.  Else out may
// alias x_new: a thread reads its 4 elements of a member row before it writes them, and no other thread touches them (a row is in one
// group once: validated on the host).  VEC: row_len % 4 == 0 and every pointer 16-byte aligned; else element by element, the last quad cut.
template <bool VEC, bool AVERAGE>
__global__ __launch_bounds__(SL_THREADS) void k_slab(const float* x_new, const float* __restrict__ y, sl_tables tab, int group0, keyed_level lv, float* out,
                                                     int64_t row_len, int64_t blocks_per_row) {
#pragma clang fp contract(off)   // s * eta, x - ., w * ., acc + .: each rounded once
  const int64_t b = (int64_t)blockIdx.x * SL_THREADS + threadIdx.x;
  if (b >= blocks_per_row) return;
  const int q = blockIdx.y;
  const int s0 = tab.start[q], s1 = tab.start[q + 1];
  const int64_t col = 4 * b;
  const int n = VEC ? 4 : (int)(row_len - col < 4 ? row_len - col : 4);
  const bool noisy = !AVERAGE && !lv.clean;
  float a = 1.f, sg = 0.f;
  if (noisy) {
    const int64_t ti = mud_level_index(lv.t, tab.member[s0], lv.toff, lv.ntab);      // the level of the group's first member
    a = lv.at[ti];
    sg = lv.st[ti];
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = s0; s < s1; ++s) {                       // table order
    const int64_t base = (int64_t)tab.member[s] * row_len + col;
    f32x4 d = quad_load<VEC>(x_new + base, n);
    if (noisy) {
      const f32x4 eta = quad_eta<VEC>(lv, tab.member[s], (uint64_t)b, base, n);
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
  const int64_t gbase = (int64_t)(group0 + q) * row_len + col;
  if constexpr (AVERAGE) {
    quad_store<VEC>(out + gbase, acc, n);
  } else {
    const f32x4 yv = quad_load<VEC>(y + gbase, n);
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ay = noisy ? a * yv[e] : yv[e];
      r[e] = acc[e] - ay;
    }
    for (int s = s0; s < s1; ++s) {
      const int64_t base = (int64_t)tab.member[s] * row_len + col;
      const f32x4 x = quad_load<VEC>(x_new + base, n);
      const float g = tab.g[s];
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float c = g * r[e];
        const float v = x[e] - c;
        o[e] = c == 0.f ? x[e] : v;                     // a correction that is 0 leaves x_new's bits (a -0 included)
      }
      quad_store<VEC>(out + base, o, n);
    }
  }
}

// the launches of one call
template <bool AVERAGE>
static int sl_run(const char* who, bool vec, const float* x, const float* y, const std::vector<sl_tables>& launches, const std::vector<int>& first_group,
                  const std::vector<int>& n_groups, const keyed_level& d, float* out, int64_t row_len, void* stream) {
  const int64_t bpr = mud_cdiv(row_len, 4);
  for (size_t i = 0; i < launches.size(); ++i) {
    vec_dispatch(vec, [&](auto v) {
      hipLaunchKernelGGL((k_slab<VEC_OF(v), AVERAGE>), dim3((unsigned)mud_cdiv(bpr, SL_THREADS), (unsigned)n_groups[i]), dim3(SL_THREADS), 0,
                         (hipStream_t)stream, x, y, launches[i], first_group[i], d, out, row_len, bpr);
    });
    MUD_CHECK_LAUNCH(who);
  }
  return MUD_OK;
}

extern "C" int mud_slab_constrain(const float* x_new, const float* y, const int32_t* members, const float* weights, const float* gains, int groups,
                                  int L, const float* noise, const int64_t* keys, uint64_t seed, int step, int kind, const int64_t* t, int toff,
                                  const float* a_tab, const float* s_tab, int ntab, int clean, float* out, int rows, int64_t row_len, void* stream) {
  keyed_level d = {noise, keys, seed, 0, t, toff, a_tab, s_tab, ntab, clean};
  MUD_REQUIRE(rows > 0 && row_len > 0, "mud_slab_constrain: bad sizes (rows %d, row_len %lld)", rows, (long long)row_len);
  MUD_REQUIRE((int64_t)rows * row_len < (1ll << 31), "mud_slab_constrain: rows * row_len must be < 2^31, got %d x %lld", rows, (long long)row_len);
  MUD_REQUIRE(groups >= 0 && groups <= rows, "mud_slab_constrain: groups must be in [0, rows = %d], got %d", rows, groups);
  MUD_REQUIRE(L >= 1 && L <= MUD_SLAB_MAX_MEMBERS, "mud_slab_constrain: L must be in [1, %d], got %d", MUD_SLAB_MAX_MEMBERS, L);
  MUD_TRY(keyed_level_word2("mud_slab_constrain", ntab, kind, step, d.word2));
  MUD_REQUIRE(x_new && out, "mud_slab_constrain: null pointer (x_new, out)");
  MUD_REQUIRE(groups == 0 || (y && members && weights && gains), "mud_slab_constrain: null pointer (y, members, weights, gains)");
  MUD_TRY(keyed_level_operands("mud_slab_constrain", groups != 0, d));
  std::vector<sl_tables> launches;
  std::vector<int> first, count;
  std::vector<uint8_t> owner;
  MUD_TRY(sl_pack("mud_slab_constrain", members, weights, gains, groups, L, rows, launches, first, count, owner));
  if (out != x_new) MUD_TRY(sl_copy_free_rows("mud_slab_constrain", x_new, out, owner, rows, row_len, stream));
  const bool vec = row_len % 4 == 0 && mud_aligned16(x_new) && mud_aligned16(out) && mud_aligned16(y) && (!noise || mud_aligned16(noise));
  return sl_run<false>("mud_slab_constrain", vec, x_new, y, launches, first, count, d, out, row_len, stream);
}

extern "C" int mud_slab_average(const float* x, const int32_t* members, const float* weights, int groups, int L, float* avg, int rows,
                                int64_t row_len, void* stream) {
  MUD_REQUIRE(rows > 0 && row_len > 0, "mud_slab_average: bad sizes (rows %d, row_len %lld)", rows, (long long)row_len);
  MUD_REQUIRE((int64_t)rows * row_len < (1ll << 31), "mud_slab_average: rows * row_len must be < 2^31, got %d x %lld", rows, (long long)row_len);
  MUD_REQUIRE(groups >= 1 && groups <= rows, "mud_slab_average: groups must be in [1, rows = %d], got %d", rows, groups);
  MUD_REQUIRE(L >= 1 && L <= MUD_SLAB_MAX_MEMBERS, "mud_slab_average: L must be in [1, %d], got %d", MUD_SLAB_MAX_MEMBERS, L);
  MUD_REQUIRE(x && members && weights && avg, "mud_slab_average: null pointer");
  std::vector<sl_tables> launches;
  std::vector<int> first, count;
  std::vector<uint8_t> owner;
  MUD_TRY(sl_pack("mud_slab_average", members, weights, nullptr, groups, L, rows, launches, first, count, owner));
  const bool vec = row_len % 4 == 0 && mud_aligned16(x) && mud_aligned16(avg);
  const keyed_level none = {nullptr, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, 1, 1};
  return sl_run<true>("mud_slab_average", vec, x, nullptr, launches, first, count, none, avg, row_len, stream);
}
