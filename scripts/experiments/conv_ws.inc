// EXPERIMENT (round 3) - not part of the shipped library: built only by
//     python scripts/build_variants.py ws:-DMUD_EXPERIMENT_WS
// and selected at run time by MUD_CONV_WS=1 on that variant.  Correct (the fp8-plan, folded-GroupNorm, statistics and wide config-3
// GPU tests pass under it) and measured NEUTRAL: 0.90-0.97x of the shipped kernel on the long reductions (384->128 at 128^2,
// 512->256 at 64^2, 320->64 at 256^2), 1.0-1.1x on most shapes, 1.3-1.4x on the 64->64 layers (profiles/r03_m_warp_specialised.txt).
// Included by conv_mfma.hip (it uses that file's helpers: cm_stage4, cm_gn_to_lds, the packed-weight constants).
// ------------------------------------------------------------------------------------------------
// Warp-specialised form of the 3x3 kernel (round 3).  The counters of k_conv_mfma (profiles/r03_d_sq_counters.txt) show the
// matrix pipe busy about half the time: every wave stages (VALU), waits and multiplies, and the two waves of a SIMD do so in
// phase.  Here the eight waves of a workgroup split the work by ROLE instead of by rows:
//   * waves 0-3, the CONSUMERS, one per SIMD, only read fragments and issue MFMAs: each owns FOUR rows x 32 px x 64 channels
//     (128 accumulator registers; twice k_conv_mfma's tile per wave, so 25 % fewer LDS fragment reads per MFMA);
//   * waves 4-7, the PRODUCERS, one per SIMD, only move data.  Wave 4 issues the weight-group DMA and nothing else: memory
//     operations of one wave retire in order, so a wave that must see its DMA land before the next barrier would drain every
//     younger-than-a-phase activation load with it; waves 5-7 fetch the raw activations TWO chunks ahead (in registers: HBM
//     latency never sits on a barrier) and run the GroupNorm / SiLU / split conversion into LDS, a third of a chunk per phase.
// A SIMD then runs one wave's MFMAs beside the other wave's vector work all the time.  Same LDS images, weight packing, phase
// structure (one workgroup barrier per 3-tap group) and epilogue as k_conv_mfma; consumer grid CWM x CWN = 4 x 1 (16 rows x 64
// channels) or 2 x 2 (8 rows x 128 channels).  Plain launches only (no fused skip conv, no split-K, no sub2).
// ------------------------------------------------------------------------------------------------
template <int CWM, int CWN>
struct CwGeo {
  static constexpr int MT = 4;                           // rows per consumer wave
  static constexpr int ROWS = CWM * MT;
  static constexpr int PW = 34;
  static constexpr int P = (ROWS + 2) * PW;
  static constexpr int PLANE = P * CM_PIX;               // one A buffer: P pixel records of one 16-channel chunk
  static constexpr int NPROD = 192;                      // staging threads (producer waves 5-7; wave 4 only moves weights)
  static constexpr int ITEMS = P * 4;                    // float4 per chunk
  static constexpr int NLOAD = (ITEMS + NPROD - 1) / NPROD;
  static constexpr int GB1 = 3 * CM_BSTEP;               // bytes per 3-tap group of ONE 64-channel tile
  static constexpr int GB = CWN * GB1;
  static constexpr int PIECES = GB / 1024;
  static constexpr int A_BYTES = 2 * PLANE;
  static constexpr int B_OFF = A_BYTES;                  // weight ring: 2 groups
  static constexpr int GN_OFF = A_BYTES + 2 * GB;
  static constexpr int EP_BYTES = 4 * (32 * 36 * 4 + 64 * 2 * 4);
  static constexpr int LDS_MAX = GN_OFF + 2 * CM_GN_MAXC * 4;
  static constexpr int lds_bytes(int gn_channels) {
    const int m = GN_OFF + 8 * ((gn_channels + 3) & ~3);
    return m > EP_BYTES ? m : EP_BYTES;
  }
  static_assert(LDS_MAX <= 160 * 1024, "LDS budget");
  static_assert(NLOAD <= 32 && NPROD % 4 == 0, "staging split");
};

#define CW_WAIT_VM(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
#define CW_WAIT_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

template <int CWM, int CWN, int PRO, int PREC>
__global__ __launch_bounds__(512, 2) void k_conv_ws(mud_conv_args a, int tiles_x, int tiles_per_img, int ntiles, int k16s, unsigned nblocks) {
  using G = CwGeo<CWM, CWN>;
  constexpr bool X8 = PREC == MUD_PREC_FP8X;
  constexpr int MT = G::MT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cm_saturating_converters();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const bool producer = __builtin_amdgcn_readfirstlane(wave) >= 4;     // wave-uniform (scalar branch)
  const int cw = wave & 3;                                              // index inside its role
  const int wm = cw % CWM, wn = cw / CWM;                               // consumer grid: CWM along pixel rows, CWN along 64-channel tiles

  unsigned lid;
  {
    const unsigned orig = blockIdx.x, xcd = orig & 7u, q = nblocks >> 3, rem = nblocks & 7u;
    lid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (orig >> 3);
  }
  const int nt = lid % ntiles;
  const unsigned rest = lid / ntiles;
  const int tile = rest % tiles_per_img;
  const int b = rest / tiles_per_img;
  const int ty0 = (tile / tiles_x) * G::ROWS, tx0 = (tile % tiles_x) * 32;
  const int64_t HW = (int64_t)a.H * a.W;
  const float* xb = a.x + (int64_t)b * HW * a.ldx;
  const int64_t tile_bytes = (int64_t)k16s * (9 * CM_BSTEP);
  const char* wb = (const char*)a.w + (int64_t)nt * CWN * tile_bytes;
  const int nchunks = k16s, total_groups = k16s * 3;
  char* const bring = smem + G::B_OFF;
  const int emul_lim = a.emul_cout > 0 ? a.emul_cout : a.Cout;
  const bool res_in_acc = a.res != nullptr;

  // ================= producer state =================
  const int ptid = (tid & 255) - 64, q = ptid & 3;        // staging thread index (producer waves 5-7: 0..191; negative in the DMA wave)
  const bool dma_wave = producer && cw == 0;
  int goff[G::NLOAD], loff[G::NLOAD];
  unsigned vmask = 0;
  f32x4 raw0[G::NLOAD], raw1[G::NLOAD];          // raw fp32 values of two chunks in flight (chunk c lives in raw{c & 1})
  f32x4 psc_r = {1.f, 1.f, 1.f, 1.f}, psh_r = {0.f, 0.f, 0.f, 0.f};
  const bool gn_fold = (PRO == MUD_PRO_AFFINE || PRO == MUD_PRO_AFFINE_SILU) && a.gn_sums != nullptr;
  const float* const gn_sc = (const float*)(smem + G::GN_OFF);
  const int gn_c = (a.Cin + 3) & ~3;
  const float* psc = a.pro_scale + (int64_t)b * a.pro_ld;
  const float* psh = a.pro_shift + (int64_t)b * a.pro_ld;
  if (producer && !dma_wave) {
#pragma unroll
    for (int j = 0; j < G::NLOAD; ++j) {
      const int item = (ptid + j * G::NPROD) % G::ITEMS;       // slots past the tile redo another thread's item (same value, same address)
      const int p = item >> 2;
      const int py = p / G::PW, px = p - py * G::PW;
      const int gy = ty0 + py - 1, gx = tx0 + px - 1;
      const bool valid = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
      goff[j] = valid ? (int)(((int64_t)gy * a.W + gx) * a.ldx) : 0;
      vmask |= (valid ? 1u : 0u) << j;
      loff[j] = p * CM_PIX + q * 8;
    }
  }
  auto fetch_raw = [&](f32x4 (&rw)[G::NLOAD], int chunk) {
    int c = chunk * 16 + q * 4;
    c = c < a.Cin ? c : 0;
#pragma unroll
    for (int j = 0; j < G::NLOAD; ++j) rw[j] = *(const f32x4*)(xb + goff[j] + c);
  };
  auto fetch_ss = [&](int chunk) {
    if (PRO == MUD_PRO_AFFINE || PRO == MUD_PRO_AFFINE_SILU) {
      int c = chunk * 16 + q * 4;
      c = c < a.Cin ? c : 0;
      // always from LDS (caller's arrays are copied there first): a choice between an LDS and a global pointer is a FLAT load, and
      // every wait behind a flat load is vmcnt(0) lgkmcnt(0)
      psc_r = *(const f32x4*)(gn_sc + c);
      psh_r = *(const f32x4*)(gn_sc + gn_c + c);
    }
  };
  auto convert = [&](f32x4 (&rw)[G::NLOAD], int chunk, char* buf, int j0, int j1) {
    const bool cvalid = chunk * 16 + q * 4 < a.Cin;
#pragma unroll
    for (int j = 0; j < G::NLOAD; ++j) {
      if (j < j0 || j >= j1) continue;
      const float keep = (cvalid && ((vmask >> j) & 1u)) ? 1.0f : 0.0f;
      h16x4 hi, lo;
      int a8 = 0, al8 = 0;
      cm_stage4<PRO, X8>(rw[j], psc_r, psh_r, keep, hi, lo, a8, al8);
      *(h16x4*)(buf + loff[j]) = hi;
      if constexpr (X8) {
        *(int*)(buf + loff[j] + 32 - q * 4) = a8;
        *(int*)(buf + loff[j] + 48 - q * 4) = al8;
      } else {
        *(h16x4*)(buf + loff[j] + 32) = lo;
      }
    }
  };
  auto dma_b = [&](int gg) {                    // weight group gg -> ring slot gg & 1 (the DMA wave moves all of it: PIECES x 1 KiB)
    if (gg >= total_groups) return;
    char* dst = bring + (gg & 1) * G::GB;
#pragma unroll
    for (int j = 0; j < G::PIECES; ++j) {
      const int piece = j;
      const int t64 = piece / (G::GB1 / 1024), within = piece % (G::GB1 / 1024);
      const char* src = wb + t64 * tile_bytes + (int64_t)gg * G::GB1 + within * 1024 + lane * 16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(dst + piece * 1024), 16, 0, 0);
    }
  };

  // The two roles run SEPARATE code from here on (same number of workgroup barriers: 2 + 3 per chunk [+ 1 with statistics]), so
  // that the register allocation is the maximum of the two paths and not their sum (128 accumulators | 2 x NLOAD raw float4).
  // the producers are the second-dispatched half of the workgroup, i.e. the losers of every issue arbitration by age
  // (MI355X_MICROARCH.md, two waves per SIMD, items 2 and 4): static priority for them, or their vector work only runs
  // when the consumer of their SIMD is parked at a barrier
  if (producer) __builtin_amdgcn_s_setprio(2);
  if (dma_wave) {
    dma_b(0);
    __builtin_amdgcn_s_barrier();
    CW_WAIT_VM(0);
    __builtin_amdgcn_s_barrier();
    for (int gg = 0; gg < total_groups; ++gg) {
      dma_b(gg + 1);                             // next group's weights (its ring slot was last read one phase ago); lands under this phase
      CW_WAIT_VM(0);
      __builtin_amdgcn_s_barrier();
    }
    if (a.stats) __builtin_amdgcn_s_barrier();
    return;
  }
  if (producer) {
    if constexpr (X8) {
      if (q == 0) {      // bytes 64..79 of every pixel record in both A buffers: the zero tap of the cross-term MFMAs
#pragma unroll
        for (int j = 0; j < G::NLOAD; ++j) {
          *(i32x4*)(smem + loff[j] + 64) = i32x4{0, 0, 0, 0};
          *(i32x4*)(smem + G::PLANE + loff[j] + 64) = i32x4{0, 0, 0, 0};
        }
      }
    }
    fetch_raw(raw0, 0);
    if (nchunks > 1) fetch_raw(raw1, 1);
    if (gn_fold) cm_gn_to_lds(a, b, ptid, G::NPROD, (float*)(smem + G::GN_OFF), gn_c);
    else if (PRO == MUD_PRO_AFFINE || PRO == MUD_PRO_AFFINE_SILU) {
      float* sc_lds = (float*)(smem + G::GN_OFF);
      for (int c = ptid; c < a.Cin; c += G::NPROD) {
        sc_lds[c] = psc[c];
        sc_lds[gn_c + c] = psh[c];
      }
    }
    CW_WAIT_LGKM0();
    __builtin_amdgcn_s_barrier();                // (GroupNorm scale / shift arrays visible to every staging thread)
    fetch_ss(0);
    convert(raw0, 0, smem, 0, G::NLOAD);
    CW_WAIT_LGKM0();
    __builtin_amdgcn_s_barrier();
    auto chunk_iter = [&](int kc, f32x4 (&nextr)[G::NLOAD], f32x4 (&freer)[G::NLOAD]) {
      // BRANCH-FREE on purpose: with control flow between the phases hipcc's waitcnt pass loses track of which registers have loads
      // pending and opens every phase with s_waitcnt vmcnt(0), draining the raw loads issued one barrier earlier (they are not needed
      // for a whole chunk).  Past the last chunk the work is redone on clamped indices into the buffer nobody reads any more.
      char* nxt = smem + ((kc + 1) & 1) * G::PLANE;
      const int kn = kc + 1 < nchunks ? kc + 1 : nchunks - 1, kf = kc + 2 < nchunks ? kc + 2 : nchunks - 1;
      fetch_ss(kn);
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        // chunk kc + 1's LDS image, a third per phase (its raw values were fetched during chunk kc - 1; A[nxt] is free all chunk long)
        convert(nextr, kn, nxt, (g * G::NLOAD) / 3, ((g + 1) * G::NLOAD) / 3);
        if (g == 0) fetch_raw(freer, kf);        // two chunks ahead (into the set chunk kc was converted from), behind this phase's conversion
        CW_WAIT_LGKM0();
        __builtin_amdgcn_s_barrier();
      }
    };
    for (int kc = 0; kc < nchunks; kc += 2) {
      chunk_iter(kc, raw1, raw0);                // chunk kc + 1 waits in raw1; chunk kc + 2 goes to raw0
      if (kc + 1 < nchunks) chunk_iter(kc + 1, raw0, raw1);
    }
    if (a.stats) __builtin_amdgcn_s_barrier();   // (keeps the consumers' statistics barrier company)
    return;
  }

  // ================= consumers =================
  const int lane_b = r * 32 + ((hh ^ ((r >> 3) & 1)) << 4);
  const int lane_a = (wm * MT * G::PW + r) * CM_PIX + hh * 16;
  const int xa_lane0 = lane_a - hh * 16 + hh * (2 * CM_PIX);
  const int xa_lane1_t0 = lane_a - hh * 16 + (hh ? 2 * CM_PIX + 64 : CM_PIX + 48);
  const int xb_lane = r * 16 + hh * (2 * CM_BSTEP);
  const int d1 = hh ? 0 : 16;
  const int s_a = (127 - CM_X_SA) * 0x01010101, s_al = (127 - CM_X_SAL) * 0x01010101;
  const int s_w = (127 - a.w_exp) * 0x01010101, s_wl = (127 - a.w_exp - 11) * 0x01010101;
  f32x16 acc[MT][2];
  if (res_in_acc) {      // the residual starts in the accumulators (see k_conv_mfma)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int co = (nt * CWN + wn) * CM_BN + n * 32 + r;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int gy = ty0 + wm * MT + m;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int gx = tx0 + (reg & 3) + 8 * (reg >> 2) + 4 * hh;
          const bool ok = gy < a.H && gx < a.W && co < a.Cout;
          acc[m][n][reg] = ok ? a.res[(((int64_t)b * a.H + gy) * a.W + gx) * a.ldr + co] : 0.f;
        }
      }
    }
  } else {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[m][n][i] = 0.f;
  }
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_s_barrier();
  for (int kc = 0; kc < nchunks; ++kc) {
    const char* cur = smem + (kc & 1) * G::PLANE;
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const int gg = kc * 3 + g;
      const char* bcur = bring + (gg & 1) * G::GB + wn * G::GB1;
#pragma unroll
      for (int sg = 0; sg < 3; ++sg) {
        h16x8 bh[2], bl[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          bh[n] = *(const h16x8*)(bcur + sg * CM_BSTEP + n * 1024 + lane_b);
          if constexpr (!X8) bl[n] = *(const h16x8*)(bcur + sg * CM_BSTEP + CM_BPLANE + n * 1024 + lane_b);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const int off = ((m + g) * G::PW + sg) * CM_PIX;
          const h16x8 ah = *(const h16x8*)(cur + lane_a + off);
          if constexpr (X8) {
            acc[m][0] = mud_mfma16(ah, bh[0], acc[m][0]);
            acc[m][1] = mud_mfma16(ah, bh[1], acc[m][1]);
          } else {
            const h16x8 al = *(const h16x8*)(cur + lane_a + off + 32);
            acc[m][0] = mud_mfma16(al, bh[0], acc[m][0]);
            acc[m][1] = mud_mfma16(al, bh[1], acc[m][1]);
            acc[m][0] = mud_mfma16(ah, bl[0], acc[m][0]);
            acc[m][1] = mud_mfma16(ah, bl[1], acc[m][1]);
            acc[m][0] = mud_mfma16(ah, bh[0], acc[m][0]);
            acc[m][1] = mud_mfma16(ah, bh[1], acc[m][1]);
          }
        }
      }
      if constexpr (X8) {
        const char* brow = bcur + xb_lane;
        const char* brow1 = bcur + CM_BSTEP + r * 16;
        const int o0 = (g * G::PW) * CM_PIX;
#pragma unroll
        for (int term = 0; term < 2; ++term) {
          const int wplane = CM_BPLANE + term * 1024, aoff = 48 - 16 * term;
          const char* pa0 = cur + xa_lane0 + o0 + aoff;
          const char* pa1 = cur + xa_lane1_t0 + o0 - d1 * term;
          const int sa = term ? s_a : s_al, sb = term ? s_wl : s_w;
          i32x8 wq[2];
#pragma unroll
          for (int n = 0; n < 2; ++n) {
            const i32x4 q0 = *(const i32x4*)(brow + wplane + n * 512);
            const i32x4 q1 = *(const i32x4*)(brow1 + wplane + n * 512);
            wq[n] = i32x8{q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3]};
          }
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const i32x4 p0 = *(const i32x4*)(pa0 + m * G::PW * CM_PIX);
            const i32x4 p1 = *(const i32x4*)(pa1 + m * G::PW * CM_PIX);
            const i32x8 aq = i32x8{p0[0], p0[1], p0[2], p0[3], p1[0], p1[1], p1[2], p1[3]};
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(aq, wq[n], acc[m][n], 0, 0, 0, sa, 0, sb);
          }
        }
      }
      // one wave per SIMD issues all the MFMAs, so nobody covers an LDS latency it waits for: pin the phase's schedule to a software
      // pipeline - 12 fragment reads up front, then two reads behind every pair of MFMAs (a read is issued >= 4 MFMAs = 128+ cycles
      // before its first use) - instead of hipcc's reads-right-before-use
      if constexpr (X8) {
        __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);
#pragma unroll
        for (int i = 0; i < 15; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 10, 0);
      } else {
        __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);
#pragma unroll
        for (int i = 0; i < 12; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 24, 0);
      }
      CW_WAIT_LGKM0();
      __builtin_amdgcn_s_barrier();
    }
  }

  // ---- epilogue (the A buffers are dead: every consumer passed the last barrier after its last fragment read)
  constexpr int EP_LD = 36;
  float* ep = (float*)smem + cw * (32 * EP_LD);
  float* st_lds = (float*)smem + 4 * (32 * EP_LD);              // [consumer wave][64 ch][2]
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int co = (nt * CWN + wn) * CM_BN + n * 32 + r;
    const bool cok = co < a.Cout;
    float badd = (a.bias && cok) ? a.bias[co] : 0.f;
    if (a.bias2 && cok) badd += a.bias2[(int64_t)b * a.bias2_ld + co];
    const int col = (lane & 7) * 4, co4 = (nt * CWN + wn) * CM_BN + n * 32 + col;
    f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, q4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) ep[((reg & 3) + 8 * (reg >> 2) + 4 * hh) * EP_LD + r] = acc[m][n][reg] + badd;
#pragma unroll
      for (int pass = 0; pass < 4; ++pass) {
        const int prow = pass * 8 + (lane >> 3);
        const int gy = ty0 + wm * MT + m, gx = tx0 + prow;
        const bool valid = gy < a.H && gx < a.W;
        const int64_t opix = ((int64_t)b * a.H + gy) * a.W + gx;
        f32x4 v = *(const f32x4*)(ep + prow * EP_LD + col);
        if (valid && co4 < a.Cout) {
          v *= a.out_scale;
          if (a.act != MUD_ACT_NONE) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = mud_act_fast(v[e], a.act);
          }
          if (a.emul && co4 < emul_lim) v *= *(const f32x4*)(a.emul + opix * a.ld_emul + co4);
          if (a.egate) {
            const f32x4 gt = *(const f32x4*)(a.egate + opix * a.ld_egate + co4);
            v = gt * v + (1.0f - gt) * *(const f32x4*)(a.eother + opix * a.ld_eother + co4);
          }
          *(f32x4*)(a.out + opix * a.ldo + co4) = v;
          s4 += v;
          q4 += v * v;
        }
      }
    }
    if (a.stats) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float ss = s4[e], qq = q4[e];
#pragma unroll
        for (int o = 8; o < 64; o <<= 1) { ss += __shfl_xor(ss, o, 64); qq += __shfl_xor(qq, o, 64); }
        if (lane < 8) {
          st_lds[(cw * 64 + n * 32 + col + e) * 2] = ss;
          st_lds[(cw * 64 + n * 32 + col + e) * 2 + 1] = qq;
        }
      }
    }
  }
  if (a.stats) {
    CW_WAIT_LGKM0();
    __builtin_amdgcn_s_barrier();
    if (tid < 128 * CWN) {
      const int tn = tid >> 7, ch = (tid & 127) >> 1, k = tid & 1, co = (nt * CWN + tn) * CM_BN + ch;
      if (co < a.Cout) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < CWM; ++w) t += st_lds[((tn * CWM + w) * 64 + ch) * 2 + k];
        atomicAdd(a.stats + ((int64_t)b * a.stats_ld + co) * 2 + k, (double)t);
      }
    }
  }
}

// the warp-specialised kernel: plain 3x3 launches that fill the chip, vector epilogue (whole aligned float4 channel columns)
static bool cm_ws_eligible(const mud_conv_args& a) {
  if (a.ks != 3 || a.skip_w || a.sub2 || a.in_up2 || a.in_s2d || (a.pro_mode != MUD_PRO_NONE && a.pro_mode != MUD_PRO_AFFINE_SILU)) return false;
  const int emul_lim = a.emul_cout > 0 ? a.emul_cout : a.Cout;
  if (((a.Cout | a.ldo | emul_lim | (a.emul ? a.ld_emul : 0) | (a.egate ? (a.ld_egate | a.ld_eother) : 0)) & 3) != 0) return false;
  if (!mud_aligned16(a.out) || (a.emul && !mud_aligned16(a.emul)) || (a.egate && (!mud_aligned16(a.egate) || !mud_aligned16(a.eother)))) return false;
  if (a.w_bstride != 0) return false;
  const int64_t n64 = mud_cdiv(a.Cout, CM_BN);
  const int64_t blocks = (n64 % 2 == 0) ? mud_cdiv(a.W, 32) * mud_cdiv(a.H, 8) * (n64 / 2) * a.B : mud_cdiv(a.W, 32) * mud_cdiv(a.H, 16) * n64 * a.B;
  return blocks >= 256 && a.H >= 8;
}

template <int CWM, int CWN, int PRO, int PREC>
static int cm_launch_ws(const mud_conv_args& a, hipStream_t s) {
  using G = CwGeo<CWM, CWN>;
  static mud_attr_once attr_once;
  if (const int rc = cm_reserve_lds(attr_once, (const void*)k_conv_ws<CWM, CWN, PRO, PREC>, G::LDS_MAX)) return rc;
  const int k16s = (int)mud_cdiv(a.Cin, 16), ntiles = (int)mud_cdiv(a.Cout, CM_BN * CWN);
  const int tiles_x = (int)mud_cdiv(a.W, 32);
  const int64_t tiles = (int64_t)tiles_x * mud_cdiv(a.H, G::ROWS);
  const int64_t nblocks = tiles * ntiles * a.B;
  MUD_REQUIRE(nblocks <= 0x7fffffff, "mud_conv2d_mfma: grid too large");
  hipLaunchKernelGGL((k_conv_ws<CWM, CWN, PRO, PREC>), dim3((unsigned)nblocks), dim3(512), G::lds_bytes((PRO == MUD_PRO_AFFINE || PRO == MUD_PRO_AFFINE_SILU) ? a.Cin : 0), s, a, tiles_x, (int)tiles,
                     ntiles, k16s, (unsigned)nblocks);
  MUD_CHECK_LAUNCH("mud_conv2d_mfma(warp-specialised)");
  return MUD_OK;
}


static bool cm_ws_wanted(const mud_conv_args& a) {
  static const bool use_ws = getenv("MUD_CONV_WS") != nullptr && atoi(getenv("MUD_CONV_WS")) != 0;
  return use_ws && a.prec == MUD_PREC_FP8X && cm_ws_eligible(a);
}
static int cm_ws_dispatch(const mud_conv_args& a, hipStream_t s) {
  const bool wide = mud_cdiv(a.Cout, CM_BN) % 2 == 0;
  if (a.pro_mode == MUD_PRO_NONE) return wide ? cm_launch_ws<2, 2, MUD_PRO_NONE, MUD_PREC_FP8X>(a, s) : cm_launch_ws<4, 1, MUD_PRO_NONE, MUD_PREC_FP8X>(a, s);
  return wide ? cm_launch_ws<2, 2, MUD_PRO_AFFINE_SILU, MUD_PREC_FP8X>(a, s) : cm_launch_ws<4, 1, MUD_PRO_AFFINE_SILU, MUD_PREC_FP8X>(a, s);
}
