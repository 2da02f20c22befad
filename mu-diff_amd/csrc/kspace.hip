// Sampling a target that was acquired undersampled in k-space (include/mudiff_hip.h: mud_fft2_c2c, mud_fft2_r2c, mud_kspace_constrain;
// mudiff_hip.kspace).  F is the unitary 2D DFT of an S x S slice, S a power of two in [16, 512], DC at [0][0],
// scale 1/S per 2D transform (an exact power of two, applied once, in the column pass).
//  - fft2: a row pass and a column pass, each a batch of line transforms in LDS;
//  - constrain: out = x_new - Re F^H[ mask ? F(x_new - s * eta) - a * y : 0 ] in three launches: rows forward (the prologue fused into
//    the load), columns forward -> residual -> columns inverse without leaving LDS, rows inverse (the epilogue fused into the store).
// A workgroup owns KS_LINES(S) whole lines from load to store, so in place is allowed; no atomics, and a slice's result is a function of
// that slice's operands alone.  Twiddles: fp64 sincospi rounded to fp32, S/2 of them per workgroup into LDS.
#include "keyed_rows.h"
#include "kspace_lines.h"       // the line transforms and the column pass, shared with slab_kspace.hip

#pragma clang fp contract(off)   // s * eta, x - p: each rounded once, as tests/kspace_ref.py states them

// what the constraint's row passes need beside the lines
struct ks_con {
  const float* x_new;
  keyed_level d;
  float* out;
};

enum { KS_ROW_FFT = 0, KS_ROW_FWD = 1, KS_ROW_INV = 2 };

// Row pass: workgroup b owns the lines b * L .. b * L + L - 1 of the rows * S lines of the batch (L divides S: never two slices).
//  KS_ROW_FFT: `in` (REAL: fp32, else complex) -> DIF with the sign of `inverse` -> data, natural order;
//  KS_ROW_FWD: d = x_new - s * eta (clean: x_new), 4 consecutive elements = one Philox block per thread -> forward DIF -> data;
//  KS_ROW_INV: data -> inverse DIT -> out = x_new - Re(.), 4 consecutive elements per thread (out may be x_new: read, then written, by
//              the same thread).
template <int MODE, bool REAL>
__global__ __launch_bounds__(KS_THREADS) void k_ks_rows(const void* in, float2* data, ks_con c, int logS, int logL, int inverse) {
  extern __shared__ float2 ks_lds[];
  const int S = 1 << logS, P = S + 1, L = 1 << logL;
  float2* x = ks_lds;
  float2* tw = ks_lds + L * P;
  const int64_t line0 = (int64_t)blockIdx.x << logL;
  ks_twiddles(tw, S);
  if constexpr (MODE == KS_ROW_FFT) {
    for (int i = threadIdx.x; i < L * S; i += KS_THREADS) {
      const int l = i >> logS, v = i & (S - 1);
      const int64_t g = ((line0 + l) << logS) + v;
      x[l * P + v] = REAL ? make_float2(reinterpret_cast<const float*>(in)[g], 0.f) : reinterpret_cast<const float2*>(in)[g];
    }
    ks_lines_dif(x, P, logL, logS, tw, inverse != 0);
    for (int i = threadIdx.x; i < L * S; i += KS_THREADS) {
      const int l = i >> logS, v = i & (S - 1);
      data[((line0 + l) << logS) + v] = x[l * P + ks_bitrev(v, logS)];
    }
  } else if constexpr (MODE == KS_ROW_FWD) {
    for (int i = threadIdx.x; i < L * (S >> 2); i += KS_THREADS) {
      const int l = i >> (logS - 2), c4 = i & ((S >> 2) - 1);
      const int64_t line = line0 + l, r = line >> logS, u = line & (S - 1);
      const int64_t g = (line << logS) + 4 * c4;
      f32x4 d = quad_load<true>(c.x_new + g, 4);
      if (!c.d.clean) {
        const float s = c.d.st[mud_level_index(c.d.t, r, c.d.toff, c.d.ntab)];
        const f32x4 eta = quad_eta<true>(c.d, r, (uint64_t)((u << (logS - 2)) + c4), g, 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = s * eta[e];
          d[e] = d[e] - p;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) x[l * P + 4 * c4 + e] = make_float2(d[e], 0.f);
    }
    ks_lines_dif(x, P, logL, logS, tw, false);
    for (int i = threadIdx.x; i < L * S; i += KS_THREADS) {
      const int l = i >> logS, v = i & (S - 1);
      data[((line0 + l) << logS) + v] = x[l * P + ks_bitrev(v, logS)];
    }
  } else {
    for (int i = threadIdx.x; i < L * S; i += KS_THREADS) {
      const int l = i >> logS, v = i & (S - 1);
      x[l * P + ks_bitrev(v, logS)] = data[((line0 + l) << logS) + v];
    }
    ks_lines_dit(x, P, logL, logS, tw, true);
    for (int i = threadIdx.x; i < L * (S >> 2); i += KS_THREADS) {
      const int l = i >> (logS - 2), c4 = i & ((S >> 2) - 1);
      const int64_t g = ((line0 + l) << logS) + 4 * c4;
      f32x4 o = *reinterpret_cast<const f32x4*>(c.x_new + g);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float re = x[l * P + 4 * c4 + e].x;
        o[e] = re == 0.f ? o[e] : o[e] - re;              // a zero correction of either sign keeps x_new's bits, -0 included
      }
      *reinterpret_cast<f32x4*>(c.out + g) = o;
    }
  }
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------------
static int ks_fft2(const char* name, const void* in, bool real, float2* out, int rows, int S, int inverse, hipStream_t stream) {
  const int logS = ks_log2(S);
  MUD_REQUIRE(logS > 0, "%s: S must be a power of two in [%d, %d], got %d", name, KS_MIN_S, KS_MAX_S, S);
  MUD_REQUIRE(rows > 0 && (int64_t)rows * S * S < (1ll << 31), "%s: rows must be > 0 with rows * S * S < 2^31, got %d", name, rows);
  MUD_REQUIRE(in && out, "%s: null pointer", name);
  MUD_REQUIRE(!real || in != (const void*)out, "%s: the real-input form cannot run in place", name);
  const int logL = ks_log_lines(S);
  const dim3 grid_rows((unsigned)(((int64_t)rows << logS) >> logL)), grid_cols((unsigned)((int64_t)rows * (S >> logL)));
  const size_t lds = ks_lds_bytes(S);
  const ks_con none = {};
  if (real)
    hipLaunchKernelGGL((k_ks_rows<KS_ROW_FFT, true>), grid_rows, dim3(KS_THREADS), lds, stream, in, out, none, logS, logL, inverse);
  else
    hipLaunchKernelGGL((k_ks_rows<KS_ROW_FFT, false>), grid_rows, dim3(KS_THREADS), lds, stream, in, out, none, logS, logL, inverse);
  MUD_CHECK_LAUNCH(name);
  hipLaunchKernelGGL((k_ks_cols<false, ks_level_own>), grid_cols, dim3(KS_THREADS), lds, stream, out, (const float2*)nullptr, (const uint8_t*)nullptr, 1,
                     (const int64_t*)nullptr, 0, (const float*)nullptr, 1, 1, logS, logL, inverse, ks_level_own{});
  MUD_CHECK_LAUNCH(name);
  return MUD_OK;
}

extern "C" int mud_fft2_c2c(const float* in, float* out, int rows, int S, int inverse, void* stream) {
  return ks_fft2("mud_fft2_c2c", in, false, reinterpret_cast<float2*>(out), rows, S, inverse, (hipStream_t)stream);
}

extern "C" int mud_fft2_r2c(const float* in, float* out, int rows, int S, int inverse, void* stream) {
  return ks_fft2("mud_fft2_r2c", in, true, reinterpret_cast<float2*>(out), rows, S, inverse, (hipStream_t)stream);
}

extern "C" int mud_kspace_constrain(const float* x_new, const float* y, const uint8_t* mask, int mask_rows, const float* noise, const int64_t* keys,
                                    uint64_t seed, int step, int kind, const int64_t* t, int toff, const float* a_tab, const float* s_tab, int ntab,
                                    int clean, float* out, float* work, int rows, int S, void* stream) {
  ks_con c = {x_new, {noise, keys, seed, 0, t, toff, a_tab, s_tab, ntab, clean}, out};
  const int logS = ks_log2(S);
  MUD_REQUIRE(logS > 0, "mud_kspace_constrain: S must be a power of two in [%d, %d], got %d", KS_MIN_S, KS_MAX_S, S);
  MUD_REQUIRE(rows > 0 && (int64_t)rows * S * S < (1ll << 31), "mud_kspace_constrain: rows must be > 0 with rows * S * S < 2^31, got %d", rows);
  MUD_REQUIRE(mask_rows == 1 || mask_rows == rows, "mud_kspace_constrain: mask_rows must be 1 or rows (%d), got %d", rows, mask_rows);
  MUD_TRY(keyed_level_word2("mud_kspace_constrain", ntab, kind, step, c.d.word2));
  MUD_REQUIRE(x_new && y && mask && out && work, "mud_kspace_constrain: null pointer (x_new, y, mask, out, work)");
  MUD_TRY(keyed_level_operands("mud_kspace_constrain", true, c.d));
  MUD_REQUIRE(mud_aligned16(x_new) && mud_aligned16(out) && (!noise || mud_aligned16(noise)) && (((uintptr_t)y | (uintptr_t)work) & 7u) == 0,
              "mud_kspace_constrain: x_new, out and noise must be 16-byte aligned, y and work 8-byte");
  MUD_REQUIRE((const void*)work != (const void*)x_new && (const void*)work != (const void*)out && (const void*)work != (const void*)y,
              "mud_kspace_constrain: work must be a buffer of its own");
  const int logL = ks_log_lines(S);
  const dim3 grid_rows((unsigned)(((int64_t)rows << logS) >> logL)), grid_cols((unsigned)((int64_t)rows * (S >> logL)));
  const size_t lds = ks_lds_bytes(S);
  hipStream_t st = (hipStream_t)stream;
  float2* w = reinterpret_cast<float2*>(work);
  hipLaunchKernelGGL((k_ks_rows<KS_ROW_FWD, false>), grid_rows, dim3(KS_THREADS), lds, st, (const void*)nullptr, w, c, logS, logL, 0);
  MUD_CHECK_LAUNCH("mud_kspace_constrain");
  hipLaunchKernelGGL((k_ks_cols<true, ks_level_own>), grid_cols, dim3(KS_THREADS), lds, st, w, reinterpret_cast<const float2*>(y), mask, mask_rows, t, toff, a_tab, ntab,
                     clean, logS, logL, 0, ks_level_own{});
  MUD_CHECK_LAUNCH("mud_kspace_constrain");
  hipLaunchKernelGGL((k_ks_rows<KS_ROW_INV, false>), grid_rows, dim3(KS_THREADS), lds, st, (const void*)nullptr, w, c, logS, logL, 1);
  MUD_CHECK_LAUNCH("mud_kspace_constrain");
  return MUD_OK;
}
