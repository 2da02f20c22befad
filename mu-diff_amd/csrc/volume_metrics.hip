// On-device scoring of a predicted volume (include/mudiff_hip.h: mud_volume_metrics; mudiff_hip.volume_metrics).
//
// Per plane of a [Z, X, Y] slab and per region (bit k of a uint8 mask per voxel), the sums that PSNR, MAE, SSIM3D and the std / error
// correlation are made of: the slice metrics of metrics.hip carried to fp32 volumes, a 7x7x7 window and masked means.
//  - window sums of x, y, x^2, y^2 and xy are formed in fp64 (the product of two fp32 values is exact there) as a fixed function of
//    the window: 7-sums along Y, then along X, then along Z, each in index order, with no running add-new / subtract-old sums.  A
//    voxel's SSIM therefore does not depend on the tiling;
//  - the SSIM expression is evaluated with contraction off, so identical inputs give exactly 1.0;
//  - partials go per (plane, region, workgroup) to a workspace and a second kernel adds them per plane in workgroup order.  No float
//    atomics: the sums are bit-identical run to run.
#include "volume_common.h"      // vi_aligned

#define VM_TC 64                          // output columns (Y) of a tile: one per lane
#define VM_TR 8                           // output rows (X) of a tile: one per wave
#define VM_THREADS (VM_TC * VM_TR)
#define VM_ZC 16                          // output planes per workgroup (it reads VM_ZC + 6 planes)
#define VM_HR (VM_TR + 6)                 // rows of a plane's tile, halo included
#define VM_HC (VM_TC + 6)                 // columns of a plane's tile, halo included
#define VM_NQ MUD_VM_NQ
#define VM_MAX_REG MUD_VM_MAX_REGIONS

// One workgroup: the VM_TR x VM_TC in-plane tile at (x0, y0) over the output planes [z0, z1).  For every plane p it reads (z0-3 ..
// z1+2): the (VM_HR x VM_HC) tile of pred and gt goes to LDS (zeros outside the volume), the 7-sums along Y of the 5 moments of every
// tile row go to LDS, and each lane adds 7 of them along X for its voxel and pushes the result into a 7-deep register ring.  The ring
// then holds planes p-6..p, so the window sums of the voxel at the centre plane c = p-3 are the ring's 7 entries added in plane order.
// Lane (wave, lane) owns voxel (x0 + wave, y0 + lane) of every output plane: its error sums, and its SSIM when the whole window lies
// in the volume.  A plane's per-region sums are reduced per wave (butterflies: every lane ends with the same bits), then over the
// waves in index order.
__global__ __launch_bounds__(VM_THREADS) void k_volume_metrics(const float* __restrict__ pred, const float* __restrict__ gt,
                                                              const uint8_t* __restrict__ region, const float* __restrict__ sd,
                                                              int Z, int X, int Y, int nreg, int ntx, int nty, double* __restrict__ part) {
  __shared__ float tp[VM_HR][VM_HC], tg[VM_HR][VM_HC];
  __shared__ double hs[5][VM_HR][VM_TC];
  __shared__ double red[VM_TR][VM_MAX_REG][VM_NQ];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int yt = blockIdx.x % nty, xt = (blockIdx.x / nty) % ntx, zc = blockIdx.x / (nty * ntx);
  const int x0 = xt * VM_TR, y0 = yt * VM_TC;
  const int xo = x0 + wave, yo = y0 + lane;
  const bool in_vox = xo < X && yo < Y;
  const bool in_plane_int = xo >= 3 && xo < X - 3 && yo >= 3 && yo < Y - 3;
  const int z0 = zc * VM_ZC, z1 = min(z0 + VM_ZC, Z);
  const int64_t plane = (int64_t)X * Y;
  const int64_t vox = (int64_t)xo * Y + yo;
  const int parts = ntx * nty, part_id = xt * nty + yt;
  const double cov_norm = 343.0 / 342.0, C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;

  double ring[7][5];
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int q = 0; q < 5; ++q) ring[k][q] = 0.0;

  for (int p = max(z0 - 3, 0); p < z1 + 3; ++p) {
    // ---- plane p into the ring (planes past the volume push zeros: they only sit in windows that are never evaluated)
    double w[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (p < Z) {                                                        // uniform over the workgroup
      const float* pp = pred + p * plane;
      const float* gp = gt + p * plane;
      for (int i = t; i < VM_HR * VM_HC; i += VM_THREADS) {
        const int rr = i / VM_HC, cc = i - rr * VM_HC;
        const int x = x0 - 3 + rr, y = y0 - 3 + cc;
        float a = 0.0f, b = 0.0f;
        if (x >= 0 && x < X && y >= 0 && y < Y) {
          a = pp[(int64_t)x * Y + y];
          b = gp[(int64_t)x * Y + y];
        }
        tp[rr][cc] = a;
        tg[rr][cc] = b;
      }
      __syncthreads();
      for (int i = t; i < VM_HR * VM_TC; i += VM_THREADS) {
        const int rr = i / VM_TC, cc = i - rr * VM_TC;
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
          const double a = tp[rr][cc + j], b = tg[rr][cc + j];
          sx += a;
          sy += b;
          sxx += a * a;
          syy += b * b;
          sxy += a * b;
        }
        hs[0][rr][cc] = sx;
        hs[1][rr][cc] = sy;
        hs[2][rr][cc] = sxx;
        hs[3][rr][cc] = syy;
        hs[4][rr][cc] = sxy;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 7; ++j)
#pragma unroll
        for (int q = 0; q < 5; ++q) w[q] += hs[q][wave + j][lane];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
      for (int q = 0; q < 5; ++q) ring[k][q] = ring[k + 1][q];
#pragma unroll
    for (int q = 0; q < 5; ++q) ring[6][q] = w[q];

    // ---- output plane c = p - 3
    const int c = p - 3;
    if (c < z0 || c >= z1) continue;                                    // uniform over the workgroup
    const bool has_ssim = in_plane_int && c >= 3 && c < Z - 3;
    double ssim = 0.0;
    if (has_ssim) {
      double S[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int q = 0; q < 5; ++q) S[q] += ring[k][q];
      {
#pragma clang fp contract(off)
        const double ux = S[0] / 343.0, uy = S[1] / 343.0;
        const double uxx = S[2] / 343.0, uyy = S[3] / 343.0, uxy = S[4] / 343.0;
        const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
        const double a1 = 2.0 * ux * uy + C1, a2 = 2.0 * vxy + C2;
        const double b1 = ux * ux + uy * uy + C1, b2 = vx + vy + C2;
        ssim = (a1 * a2) / (b1 * b2);
      }
    }
    float pv = 0.0f, gv = 0.0f, sv = 0.0f;
    unsigned m = 0u;
    if (in_vox) {
      const int64_t idx = (int64_t)c * plane + vox;
      pv = pred[idx];
      gv = gt[idx];
      m = region[idx];
      if (sd) sv = sd[idx];
    }
    const double d = (double)pv - (double)gv, e = fabs(d), s = sv;
    __syncthreads();                                                    // the previous output plane's readers of red are done
    for (int k = 0; k < nreg; ++k) {
      const bool in = (m >> k) & 1u;
      const unsigned long long bal = __ballot(in), bal_i = __ballot(in && has_ssim);
      double v[VM_NQ];
#pragma unroll
      for (int q = 0; q < VM_NQ; ++q) v[q] = 0.0;
      v[MUD_VM_N] = (double)__popcll(bal);
      v[MUD_VM_N_INT] = (double)__popcll(bal_i);
      if (bal) {                                                        // uniform over the wave
        v[MUD_VM_SSE] = mud_wave_sum(in ? d * d : 0.0);
        v[MUD_VM_SAE] = mud_wave_sum(in ? e : 0.0);
        if (bal_i) v[MUD_VM_SSIM] = mud_wave_sum(in && has_ssim ? ssim : 0.0);
        if (sd) {
          v[MUD_VM_SS] = mud_wave_sum(in ? s : 0.0);
          v[MUD_VM_SS2] = mud_wave_sum(in ? s * s : 0.0);
          v[MUD_VM_SSE_STD] = mud_wave_sum(in ? s * e : 0.0);
        }
      }
      if (lane == 0) {
#pragma unroll
        for (int q = 0; q < VM_NQ; ++q) red[wave][k][q] = v[q];
      }
    }
    __syncthreads();
    if (t < nreg * VM_NQ) {
      const int k = t / VM_NQ, q = t - k * VM_NQ;
      double acc = 0.0;
#pragma unroll
      for (int wv = 0; wv < VM_TR; ++wv) acc += red[wv][k][q];
      part[(((int64_t)c * nreg + k) * parts + part_id) * VM_NQ + q] = acc;
    }
  }
}

// one lane per (plane, region, quantity): the plane's partials in workgroup order
__global__ __launch_bounds__(256) void k_volume_metrics_final(const double* __restrict__ part, int64_t n, int parts, double* __restrict__ sums) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t pr = i / VM_NQ, q = i - pr * VM_NQ;
  double acc = 0.0;
  for (int k = 0; k < parts; ++k) acc += part[(pr * parts + k) * VM_NQ + q];
  sums[i] = acc;
}

static void vm_grid(int Z, int X, int Y, int64_t& ntx, int64_t& nty, int64_t& nzc) {
  ntx = mud_cdiv(X, VM_TR);
  nty = mud_cdiv(Y, VM_TC);
  nzc = mud_cdiv(Z, VM_ZC);
}

extern "C" int64_t mud_volume_metrics_ws_bytes(int Z, int X, int Y, int nreg) {
  if (Z < 7 || X < 7 || Y < 7 || nreg < 1 || nreg > VM_MAX_REG) return -1;
  int64_t ntx, nty, nzc;
  vm_grid(Z, X, Y, ntx, nty, nzc);
  return (int64_t)Z * nreg * ntx * nty * VM_NQ * 8;
}

extern "C" int mud_volume_metrics(const float* pred, const float* gt, const uint8_t* region, const float* std, int Z, int X, int Y, int nreg,
                                  double* sums, void* ws, int64_t ws_bytes, void* stream) {
  MUD_REQUIRE(Z >= 7 && X >= 7 && Y >= 7, "mud_volume_metrics: need Z, X, Y >= 7 (the SSIM window; got %d x %d x %d)", Z, X, Y);
  MUD_REQUIRE(nreg >= 1 && nreg <= VM_MAX_REG, "mud_volume_metrics: nreg must be in [1, %d] (got %d)", VM_MAX_REG, nreg);
  MUD_REQUIRE((int64_t)X * Y <= (1ll << 40), "mud_volume_metrics: plane too large (%d x %d)", X, Y);
  MUD_REQUIRE(pred && gt && region && sums && ws, "mud_volume_metrics: null pointer");
  MUD_REQUIRE(ws_bytes >= mud_volume_metrics_ws_bytes(Z, X, Y, nreg), "mud_volume_metrics: ws holds %lld bytes, needs %lld",
              (long long)ws_bytes, (long long)mud_volume_metrics_ws_bytes(Z, X, Y, nreg));
  MUD_REQUIRE(vi_aligned(ws, 8) && vi_aligned(sums, 8), "mud_volume_metrics: ws and sums must be 8-byte aligned");
  int64_t ntx, nty, nzc;
  vm_grid(Z, X, Y, ntx, nty, nzc);
  const int64_t blocks = ntx * nty * nzc, n = (int64_t)Z * nreg * VM_NQ;
  MUD_REQUIRE(blocks <= 0x7fffffff, "mud_volume_metrics: too many workgroups (%lld)", (long long)blocks);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_volume_metrics, dim3((unsigned)blocks), dim3(VM_THREADS), 0, st, pred, gt, region, std, Z, X, Y, nreg, (int)ntx,
                     (int)nty, (double*)ws);
  hipLaunchKernelGGL(k_volume_metrics_final, dim3((unsigned)mud_cdiv(n, 256)), dim3(256), 0, st, (const double*)ws, n, (int)(ntx * nty), sums);
  MUD_CHECK_LAUNCH("mud_volume_metrics");
  return MUD_OK;
}
