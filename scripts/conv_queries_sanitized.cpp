// Host-side queries of the matrix-core conv dispatcher under AddressSanitizer + UBSan, stand-alone: no GPU, nothing is launched.
// Links csrc/conv_mfma.hip and csrc/api.cpp compiled with the sanitizers on the HOST side only:
//   cd mu-diff_amd/csrc && S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined" && T=$(mktemp -d) &&
//   hipcc $(make -s print-flags-conv_mfma) $S -c conv_mfma.hip -o $T/conv_mfma.o &&
//   hipcc $(make -s print-flags-api) $S -c api.cpp -o $T/api.o &&
//   hipcc $(make -s print-flags-api) $S -I../../include -c ../../scripts/conv_queries_sanitized.cpp -o $T/main.o &&
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined $T/main.o $T/api.o $T/conv_mfma.o -o $T/conv_queries_sanitized && $T/conv_queries_sanitized
// The table is tests/test_conv_tiles_host.py's (written by hand from the rule, both sides of every threshold); the checks are that
// file's: the tile, which plan is built where, in_up2 / in_s2d at the size they run at, the split-K workspace of the tile the query names.
#include <cstdio>
#include <cstring>
#include "mudiff_hip.h"

enum { T8X2 = MUD_TILE_8X2, T16X1 = MUD_TILE_16X1, MT2 = MUD_TILE_MT2, MT1 = MUD_TILE_MT1, T8X1R = MUD_TILE_8X1R };
struct Row { int B, H, W, Cin, Cout, skip, tile; };
static const Row kTable[] = {
    {128, 11, 35, 20, 60, 0, T8X1R}, {127, 11, 35, 20, 60, 0, MT1}, {128, 7, 35, 20, 60, 0, MT1}, {256, 8, 35, 20, 60, 0, T8X1R},
    {256, 7, 35, 20, 60, 0, MT1}, {128, 11, 33, 20, 60, 0, T8X1R}, {128, 11, 32, 20, 60, 0, MT1}, {128, 11, 35, 64, 60, 0, T8X1R},
    {128, 11, 35, 68, 60, 0, MT2}, {128, 11, 35, 20, 64, 0, T8X1R}, {128, 11, 35, 20, 68, 0, T8X2},
    {64, 11, 35, 24, 100, 0, T8X2}, {63, 11, 35, 24, 100, 0, MT1}, {128, 8, 35, 24, 100, 0, T8X2}, {128, 7, 35, 24, 100, 0, MT1},
    {64, 19, 35, 24, 100, 0, T8X2}, {22, 19, 35, 24, 260, 0, T16X1},
    {64, 19, 35, 68, 60, 0, T16X1}, {63, 19, 35, 68, 60, 0, MT1}, {64, 15, 35, 68, 60, 0, MT1}, {128, 16, 35, 68, 60, 0, T16X1},
    {128, 15, 35, 68, 60, 0, MT2}, {43, 19, 35, 36, 132, 0, T16X1}, {22, 19, 35, 36, 132, 0, T16X1}, {21, 19, 35, 36, 132, 0, MT1},
    {127, 11, 35, 68, 60, 0, MT1}, {86, 11, 35, 68, 60, 0, MT1},
    {128, 11, 35, 20, 60, 1, MT1}, {128, 11, 35, 68, 60, 1, MT1}, {64, 11, 35, 24, 100, 1, T8X2}, {64, 19, 35, 68, 60, 1, T16X1}, {63, 19, 35, 68, 60, 1, MT1},
    {2, 256, 256, 64, 64, 0, T8X1R}, {4, 128, 128, 96, 128, 0, T8X2}, {2, 256, 256, 80, 64, 0, T16X1}, {64, 8, 256, 68, 64, 0, MT2},
    {1, 20, 37, 48, 96, 0, MT1}, {2, 33, 70, 32, 64, 0, MT1},
    {4, 128, 128, 64, 128, 1, T8X2}, {2, 256, 256, 48, 64, 1, T16X1}, {2, 20, 37, 48, 96, 1, MT1}, {1, 64, 64, 512, 256, 1, MT1},
    {16, 64, 64, 384, 256, 1, T8X2}, {8, 128, 128, 192, 64, 1, T16X1}, {2, 33, 70, 320, 64, 1, MT1}, {3, 16, 16, 24, 40, 1, MT1},
    {2, 11, 35, 20, 60, 0, MT1}, {128, 5, 35, 20, 60, 0, MT1}, {128, 11, 35, 20, 62, 0, T8X1R}, {64, 11, 35, 24, 102, 0, T8X2},
    {64, 19, 35, 68, 62, 0, T16X1}, {128, 11, 35, 68, 62, 0, MT2}, {1, 13, 35, 260, 68, 0, MT1},
};

static int failures = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      ++failures;                            \
      printf("FAILED %s: ", #cond);          \
      printf(__VA_ARGS__);                   \
      printf("\n");                          \
    }                                        \
  } while (0)

static float buf[64] __attribute__((aligned(16)));

static mud_conv_args launch3(int B, int H, int W, int Cin, int Cout) {
  mud_conv_args a;
  memset(&a, 0, sizeof a);
  a.x = buf, a.out = buf;
  a.B = B, a.H = H, a.W = W, a.Cin = Cin, a.ldx = Cin, a.ks = 3, a.stride = 1, a.pad = 1, a.Cout = Cout, a.ldo = (Cout + 3) & ~3;
  return a;
}

int main() {
  for (const Row& r : kTable) {
    mud_conv_args a = launch3(r.B, r.H, r.W, r.Cin, r.Cout);
    if (r.skip) a.skip_w = buf, a.pro_mode = MUD_PRO_AFFINE_SILU;
    const int tile = mud_conv2d_mfma_tile(&a);
    CHECK(tile == r.tile, "%dx%dx%d %d->%d skip=%d: tile %d, the rule gives %d", r.B, r.H, r.W, r.Cin, r.Cout, r.skip, tile, r.tile);
    const bool big = tile == T8X2 || tile == T16X1 || tile == T8X1R;
    for (int mode = MUD_PRO_NONE; mode <= MUD_PRO_LRELU; ++mode) {
      a.pro_mode = mode;
      const bool built = mode == MUD_PRO_AFFINE_SILU || (mode == MUD_PRO_NONE && !r.skip);
      CHECK(mud_conv2d_mfma_prec_supported(&a, MUD_PREC_FP8X) == (big && built), "fp8x, mode %d, %dx%dx%d %d->%d skip=%d", mode, r.B, r.H, r.W, r.Cin, r.Cout, r.skip);
      CHECK(mud_conv2d_mfma_prec_supported(&a, MUD_PREC_16X1) == (!r.skip || mode == MUD_PRO_AFFINE_SILU), "16x1, mode %d", mode);
      CHECK(mud_conv2d_mfma_prec_supported(&a, MUD_PREC_16X3) == 1, "16x3, mode %d", mode);
      a.sub2 = 1;
      CHECK(mud_conv2d_mfma_prec_supported(&a, MUD_PREC_FP8X) == 0, "fp8x with sub2, mode %d", mode);
      a.sub2 = 0;
    }
    CHECK(mud_conv2d_mfma_prec_supported(&a, 3) == 0 && mud_conv2d_mfma_prec_supported(&a, -1) == 0, "an unknown plan");
    (void)mud_conv2d_mfma_splitk_bytes(&a);
    (void)mud_conv2d_mfma_res_up2_supported(&a);
  }
  // what is not a 3x3 launch has no tile; out-of-range prologue / plan codes index nothing
  CHECK(mud_conv2d_mfma_tile(nullptr) == -1, "null");
  // (4 and 5 key the in_up2 / in_s2d rows of the table and are no values of pro_mode: asked on the two tiles those rows exist for -
  // 4x128x128 96->128 is 8X2, 1x20x37 48->96 is MT1 - and on 8X1R, which has none)
  for (const Row& r : {Row{128, 11, 35, 20, 60, 0, T8X1R}, Row{4, 128, 128, 96, 128, 0, T8X2}, Row{1, 20, 37, 48, 96, 0, MT1}, Row{4, 128, 128, 64, 128, 0, T8X2}}) {
    mud_conv_args a = launch3(r.B, r.H, r.W, r.Cin, r.Cout);
    CHECK(mud_conv2d_mfma_tile(&a) == r.tile, "tile of %dx%dx%d %d->%d", r.B, r.H, r.W, r.Cin, r.Cout);
    a.ks = 1;
    CHECK(mud_conv2d_mfma_tile(&a) == -1, "ks = 1");
    CHECK(mud_conv2d_mfma_prec_supported(&a, MUD_PREC_16X3) == 1 && !mud_conv2d_mfma_prec_supported(&a, MUD_PREC_16X1) && !mud_conv2d_mfma_prec_supported(&a, MUD_PREC_FP8X), "ks = 1 plans");
    a.ks = 3;
    for (int bad : {-7, 4, 5, 6, 1 << 30}) {
      a.pro_mode = bad;
      CHECK(!mud_conv2d_mfma_prec_supported(&a, MUD_PREC_16X1) && !mud_conv2d_mfma_prec_supported(&a, MUD_PREC_FP8X), "pro_mode %d on tile %d", bad, r.tile);
      a.in_up2 = 1, a.prec = bad;
      CHECK(mud_conv2d_mfma_tile(&a) == -1 && !mud_conv2d_mfma_in_up2_supported(&a) && !mud_conv2d_mfma_in_s2d_supported(&a), "prec %d", bad);
      a.in_up2 = 0, a.prec = 0;
    }
  }
  // in_up2 (asked at the output size) and in_s2d (at the folded size): 8X2 and MT1 only; in_s2d under the two fp16 plans only
  {
    mud_conv_args a = launch3(4, 128, 128, 96, 128);
    a.pro_mode = MUD_PRO_AFFINE_SILU, a.in_up2 = 1;
    CHECK(mud_conv2d_mfma_tile(&a) == T8X2 && mud_conv2d_mfma_in_up2_supported(&a), "in_up2 8X2");
    a.prec = MUD_PREC_FP8X;
    CHECK(mud_conv2d_mfma_tile(&a) == T8X2 && mud_conv2d_mfma_in_up2_supported(&a), "in_up2 8X2 fp8x");
    a.B = 1;
    CHECK(mud_conv2d_mfma_tile(&a) == -1 && !mud_conv2d_mfma_in_up2_supported(&a), "in_up2 MT1 fp8x");
    a.prec = MUD_PREC_16X1;
    CHECK(mud_conv2d_mfma_tile(&a) == MT1 && mud_conv2d_mfma_in_up2_supported(&a), "in_up2 MT1 16x1");
    mud_conv_args b = launch3(2, 256, 256, 80, 64);
    b.pro_mode = MUD_PRO_AFFINE_SILU, b.in_up2 = 1;
    CHECK(mud_conv2d_mfma_tile(&b) == -1 && !mud_conv2d_mfma_in_up2_supported(&b), "in_up2 16X1");
    mud_conv_args c = launch3(4, 128, 128, 64, 128);
    c.ldx = 16, c.in_s2d = 1;
    CHECK(mud_conv2d_mfma_tile(&c) == T8X2 && mud_conv2d_mfma_in_s2d_supported(&c), "in_s2d 8X2");
    c.prec = MUD_PREC_FP8X;
    CHECK(mud_conv2d_mfma_tile(&c) == -1 && !mud_conv2d_mfma_in_s2d_supported(&c), "in_s2d fp8x");
    c.prec = MUD_PREC_16X1, c.B = 1;
    CHECK(mud_conv2d_mfma_tile(&c) == MT1 && mud_conv2d_mfma_in_s2d_supported(&c), "in_s2d MT1 16x1");
    c.B = 8, c.Cout = 64, c.ldo = 64;
    CHECK(mud_conv2d_mfma_tile(&c) == -1 && !mud_conv2d_mfma_in_s2d_supported(&c), "in_s2d 8X1R");
  }
  // the split-K workspace is sized for the tile the query names: MT1, 256 threads x 32 accumulators; the fused skip conv twice that
  {
    mud_conv_args a = launch3(1, 13, 35, 260, 68);
    const long long blocks = 2 * 4 * 2 * 1;
    CHECK(mud_conv2d_mfma_splitk_bytes(&a) == 4 * blocks * 256 * 32 * 4, "MT1 slabs: %lld", (long long)mud_conv2d_mfma_splitk_bytes(&a));
    a.skip_w = buf, a.pro_mode = MUD_PRO_AFFINE_SILU;
    CHECK(mud_conv2d_mfma_splitk_bytes(&a) == 0, "fused, no arrival counters");
    a.splitk_counters = (unsigned*)buf, a.splitk_ncounters = 16;
    CHECK(mud_conv2d_mfma_splitk_bytes(&a) == 2 * 4 * blocks * 256 * 32 * 4, "fused slabs");
  }
  // the dispatcher refuses, before any launch, what no row of its table holds (no device is needed to be told so)
  {
    mud_conv_args a = launch3(2, 11, 35, 20, 60);
    a.w = buf, a.prec = MUD_PREC_FP8X;
    CHECK(mud_conv2d_mfma(&a, nullptr) == MUD_ERR_ARG && strstr(mud_last_error(), "MUD_PREC_FP8X is not built"), "%s", mud_last_error());
    a.ks = 1, a.pad = 0, a.prec = MUD_PREC_16X1;
    CHECK(mud_conv2d_mfma(&a, nullptr) == MUD_ERR_ARG && strstr(mud_last_error(), "MUD_PREC_16X1"), "%s", mud_last_error());
  }
  printf(failures ? "%d checks FAILED\n" : "conv queries: every check passed (%d failures)\n", failures);
  return failures != 0;
}
