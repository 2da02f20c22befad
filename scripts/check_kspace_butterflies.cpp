// Host check of csrc/kspace_fft.h: runs the butterflies of the line transforms one by one, in the order kspace.hip's ks_lines_dif /
// ks_lines_dit issue them, and compares with a direct fp64 DFT for every supported S.  No GPU is touched.
//   hipcc --offload-arch=gfx950 -O1 -I mu-diff_amd/csrc scripts/check_kspace_butterflies.cpp -o /tmp/check_kspace && /tmp/check_kspace
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "kspace_fft.h"

static void dif(std::vector<float2>& x, int logS, const float2* tw, bool conj) {
  const int S = 1 << logS;
  for (int lq = logS - 2; lq >= 0; lq -= 2)
    for (int g = 0; g < S / 4; ++g) ks_dif4(x.data(), g, lq, logS, tw, conj);
  if (logS & 1)
    for (int g = 0; g < S / 2; ++g) ks_bfly2(x.data(), g);
}

static void dit(std::vector<float2>& x, int logS, const float2* tw, bool conj) {
  const int S = 1 << logS;
  if (logS & 1)
    for (int g = 0; g < S / 2; ++g) ks_bfly2(x.data(), g);
  for (int lq = logS & 1; lq <= logS - 2; lq += 2)
    for (int g = 0; g < S / 4; ++g) ks_dit4(x.data(), g, lq, logS, tw, conj);
}

int main() {
  const double pi = 3.14159265358979323846;
  int bad = 0;
  for (int logS = 4; logS <= 9; ++logS) {
    const int S = 1 << logS;
    std::vector<float2> tw(S / 2), in(S), a(S), b(S);
    for (int m = 0; m < S / 2; ++m) tw[m] = make_float2((float)std::cos(2 * pi * m / S), (float)-std::sin(2 * pi * m / S));
    srand(logS);
    for (auto& v : in) v = make_float2(rand() / (float)RAND_MAX - 0.5f, rand() / (float)RAND_MAX - 0.5f);
    for (int inverse = 0; inverse < 2; ++inverse) {
      std::vector<double> re(S), im(S);
      double norm = 0;
      for (int u = 0; u < S; ++u) {
        double sr = 0, si = 0;
        for (int k = 0; k < S; ++k) {
          const double ang = (inverse ? 2 : -2) * pi * (double)((long)u * k % S) / S;
          sr += in[k].x * std::cos(ang) - in[k].y * std::sin(ang);
          si += in[k].x * std::sin(ang) + in[k].y * std::cos(ang);
        }
        re[u] = sr, im[u] = si, norm += sr * sr + si * si;
      }
      a = in;
      dif(a, logS, tw.data(), inverse);
      for (int v = 0; v < S; ++v) b[ks_bitrev(v, logS)] = in[v];
      dit(b, logS, tw.data(), inverse);
      double ea = 0, eb = 0;
      for (int u = 0; u < S; ++u) {
        const float2 va = a[ks_bitrev(u, logS)], vb = b[u];
        ea += (va.x - re[u]) * (va.x - re[u]) + (va.y - im[u]) * (va.y - im[u]);
        eb += (vb.x - re[u]) * (vb.x - re[u]) + (vb.y - im[u]) * (vb.y - im[u]);
      }
      ea = std::sqrt(ea / norm), eb = std::sqrt(eb / norm);
      const double bound = 8.0 * logS * std::ldexp(1.0, -24);
      printf("S %3d inverse %d: DIF rel L2 %.3e, DIT rel L2 %.3e (bound %.3e)\n", S, inverse, ea, eb, bound);
      bad += !(ea <= bound) + !(eb <= bound);
    }
    a = in;                                                  // DIF forward, then DIT inverse on the bit-reversed result: the identity times S
    dif(a, logS, tw.data(), false);
    dit(a, logS, tw.data(), true);
    double e = 0, n = 0;
    for (int k = 0; k < S; ++k) {
      e += std::pow(a[k].x / S - in[k].x, 2) + std::pow(a[k].y / S - in[k].y, 2);
      n += in[k].x * in[k].x + in[k].y * in[k].y;
    }
    printf("S %3d round trip without a permutation: rel L2 %.3e\n", S, std::sqrt(e / n));
    bad += !(std::sqrt(e / n) <= 16.0 * logS * std::ldexp(1.0, -24));
  }
  printf(bad ? "FAILED (%d)\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
