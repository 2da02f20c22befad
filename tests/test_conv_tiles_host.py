"""CPU: which workgroup tile a 3x3 matrix-core launch runs on (mud_conv2d_mfma_tile, ops.conv_tile).  The table below is written by
hand from the rule as the comments of cm_variant3 (csrc/conv_mfma.hip) state it - it is NOT computed by a copy of that code - and holds
every threshold from both sides, so a moved threshold fails here instead of silently turning the per-tile GPU tests into tests of one
tile.  The rule, with tx = ceil(W / 32) and n = ceil(Cout / 64) 64-channel tiles, first match wins:
  8X1R  plain launch, n == 1, Cin <= 64, H >= 8 and tx * ceil(H / 8) * B >= 512
  8X2   n even, H >= 8 and tx * ceil(H / 8) * (n / 2) * B >= 256
  16X1  H >= 16 and tx * ceil(H / 16) * n * B >= 256
  MT2   H >= 8 and tx * ceil(H / 8) * n * B >= 512
  MT1   everything else
and the fused skip conv (skip_w) is built for 8X2, 16X1 and MT1 only: where a plain launch takes MT2 or 8X1R it takes MT1.
No knob of the dispatcher (MUD_CONV_MT, MUD_CONV_NO16, MUD_CONV_NO8X1R, the split-K ones) is set: they are read once per process."""
import ctypes as C
import os

import pytest
import torch

T8X2, T16X1, MT2, MT1, T8X1R = '8X2', '16X1', 'MT2', 'MT1', '8X1R'

# (B, H, W, Cin, Cout, skip) -> tile.  The arithmetic of each row is in its comment.
TABLE = [
    # ---- the one-row tile: 2 column tiles x 2 row groups x B
    ((128, 11, 35, 20, 60, False), T8X1R),      # 2 * 2 * 128 = 512
    ((127, 11, 35, 20, 60, False), MT1),        # 508 < 512: neither 8X1R nor MT2; n odd; H < 16
    ((128, 7, 35, 20, 60, False), MT1),         # H < 8
    ((256, 8, 35, 20, 60, False), T8X1R),       # H == 8: 2 * 1 * 256 = 512
    ((256, 7, 35, 20, 60, False), MT1),         # H < 8 at the same batch
    ((128, 11, 33, 20, 60, False), T8X1R),      # W = 33 is two column tiles
    ((128, 11, 32, 20, 60, False), MT1),        # W = 32 is one: 256 workgroups
    ((128, 11, 35, 64, 60, False), T8X1R),      # Cin == 64 still
    ((128, 11, 35, 68, 60, False), MT2),        # Cin > 64: 512 workgroups of the 8-row 4-wave tile
    ((128, 11, 35, 20, 64, False), T8X1R),      # Cout == 64: one channel tile
    ((128, 11, 35, 20, 68, False), T8X2),       # Cout = 68: two channel tiles, 2 * 2 * 1 * 128 = 512 >= 256
    # ---- 8 rows x 128 channels
    ((64, 11, 35, 24, 100, False), T8X2),       # 2 * 2 * 1 * 64 = 256
    ((63, 11, 35, 24, 100, False), MT1),        # 252 < 256; H < 16; MT2: 2 * 2 * 2 * 63 = 504 < 512
    ((128, 8, 35, 24, 100, False), T8X2),       # H == 8: 2 * 1 * 1 * 128 = 256
    ((128, 7, 35, 24, 100, False), MT1),        # H < 8
    ((64, 19, 35, 24, 100, False), T8X2),       # before 16X1, which would fill the chip too (2 * 2 * 2 * 64 = 512)
    ((22, 19, 35, 24, 260, False), T16X1),      # n = 5 is odd: no 8X2; 2 * 2 * 5 * 22 = 440
    # ---- 16 rows x 64 channels
    ((64, 19, 35, 68, 60, False), T16X1),       # 2 * 2 * 1 * 64 = 256
    ((63, 19, 35, 68, 60, False), MT1),         # 252 < 256; MT2: 2 * 3 * 63 = 378 < 512
    ((64, 15, 35, 68, 60, False), MT1),         # H < 16; MT2: 2 * 2 * 64 = 256 < 512
    ((128, 16, 35, 68, 60, False), T16X1),      # H == 16: 2 * 1 * 128 = 256
    ((128, 15, 35, 68, 60, False), MT2),        # H < 16 at the same batch: 2 * 2 * 128 = 512
    ((43, 19, 35, 36, 132, False), T16X1),      # n = 3: 2 * 2 * 3 * 43 = 516
    ((22, 19, 35, 36, 132, False), T16X1),      # 2 * 2 * 3 * 22 = 264
    ((21, 19, 35, 36, 132, False), MT1),        # 252 < 256; MT2: 2 * 3 * 3 * 21 = 378 < 512
    # ---- 8 rows x 64 channels, four waves
    ((127, 11, 35, 68, 60, False), MT1),        # 508 < 512
    ((86, 11, 35, 68, 60, False), MT1),         # 344
    # ---- the fused skip conv
    ((128, 11, 35, 20, 60, True), MT1),         # 8X1R -> MT1
    ((128, 11, 35, 68, 60, True), MT1),         # MT2 -> MT1
    ((64, 11, 35, 24, 100, True), T8X2),
    ((64, 19, 35, 68, 60, True), T16X1),
    ((63, 19, 35, 68, 60, True), MT1),
    # ---- the shapes the GPU tests name a tile for: test_fp16_plan_gpu.CASES ...
    ((2, 256, 256, 64, 64, False), T8X1R),      # 8 * 32 * 2 = 512
    ((4, 128, 128, 96, 128, False), T8X2),      # 4 * 16 * 1 * 4 = 256
    ((2, 256, 256, 80, 64, False), T16X1),      # Cin > 64; 8 * 16 * 2 = 256
    ((64, 8, 256, 68, 64, False), MT2),         # H < 16; 8 * 1 * 64 = 512
    ((1, 20, 37, 48, 96, False), MT1),
    ((2, 33, 70, 32, 64, False), MT1),
    # ... test_fp16_plan_gpu.test_fused_skip_launch ...
    ((4, 128, 128, 64, 128, True), T8X2),
    ((2, 256, 256, 48, 64, True), T16X1),
    ((2, 20, 37, 48, 96, True), MT1),
    ((1, 64, 64, 512, 256, True), MT1),
    # ... test_gpu_parity.test_conv_with_fused_skip_conv ('the three tile variants (8x2, 16x1, 4-row)') ...
    ((16, 64, 64, 384, 256, True), T8X2),       # 2 * 8 * 2 * 16 = 512
    ((8, 128, 128, 192, 64, True), T16X1),      # 4 * 8 * 1 * 8 = 256
    ((2, 33, 70, 320, 64, True), MT1),
    ((3, 16, 16, 24, 40, True), MT1),
    # ... and test_conv_forms_gpu
    ((2, 11, 35, 20, 60, False), MT1),
    ((128, 5, 35, 20, 60, False), MT1),
    ((128, 11, 35, 20, 62, False), T8X1R),
    ((64, 11, 35, 24, 102, False), T8X2),
    ((64, 19, 35, 68, 62, False), T16X1),
    ((128, 11, 35, 68, 62, False), MT2),
    ((1, 13, 35, 260, 68, False), MT1),
]


def _lib():
    import mudiff_hip
    if not os.path.isfile(mudiff_hip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return mudiff_hip.load()


def _view(B, H, W, Cin):
    from mudiff_hip import ops
    return ops.View(torch.empty(16), B, H, W, Cin)          # (only sizes are looked at)


def _code(name):
    import mudiff_hip
    return dict(zip((T8X2, T16X1, MT2, MT1, T8X1R), (mudiff_hip.TILE_8X2, mudiff_hip.TILE_16X1, mudiff_hip.TILE_MT2, mudiff_hip.TILE_MT1,
                                                    mudiff_hip.TILE_8X1R)))[name]


def test_tile_constants_are_the_headers():
    import re
    import mudiff_hip
    from conftest import REPO
    txt = open(os.path.join(REPO, 'include', 'mudiff_hip.h')).read()
    hdr = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define MUD_TILE_(\w+) (\d+)', txt)}
    assert hdr == {'8X2': mudiff_hip.TILE_8X2, '16X1': mudiff_hip.TILE_16X1, 'MT2': mudiff_hip.TILE_MT2, 'MT1': mudiff_hip.TILE_MT1,
                   '8X1R': mudiff_hip.TILE_8X1R}
    assert len(set(hdr.values())) == 5
    from mudiff_hip import ops
    assert ops.TILE_NAMES == {v: k for k, v in hdr.items()}


@pytest.mark.parametrize('shape,tile', TABLE, ids=[f'{"x".join(map(str, k[:3]))}_{k[3]}to{k[4]}{"_skip" if k[5] else ""}' for k, _ in TABLE])
def test_tile_of_the_hand_written_table(shape, tile):
    from mudiff_hip import ops
    _lib()
    B, H, W, Cin, Cout, skip = shape
    got = ops.conv_tile(_view(B, H, W, Cin), Cout, skip=skip, pro_mode=ops.PRO_AFFINE_SILU if skip else ops.PRO_NONE)
    assert got == _code(tile), f'{shape}: the dispatcher takes {ops.TILE_NAMES.get(got, got)}, the documented rule gives {tile}'


def test_every_tile_and_both_sides_of_every_threshold_are_in_the_table():
    assert {t for _, t in TABLE} == {T8X2, T16X1, MT2, MT1, T8X1R}
    assert {t for k, t in TABLE if k[5]} == {T8X2, T16X1, MT1}
    assert len({k for k, _ in TABLE}) == len(TABLE)


def test_fp8x_plan_is_built_exactly_on_the_eight_wave_tiles():
    """mud_conv2d_mfma_prec_supported(FP8X) is true exactly on 8X2, 16X1 and 8X1R, for the prologues the plan is built for (none and
    AdaGN + SiLU; the fused skip conv: AdaGN + SiLU only), never with sub2; MUD_PREC_16X1 and 16X3 do not depend on the tile."""
    from mudiff_hip import ops
    _lib()
    for (B, H, W, Cin, Cout, skip), tile in TABLE:
        xv = _view(B, H, W, Cin)
        big = ops.conv_tile(xv, Cout, skip=skip) in (_code(T8X2), _code(T16X1), _code(T8X1R))       # (the query's answer, not the table's)
        for mode in (ops.PRO_NONE, ops.PRO_AFFINE, ops.PRO_AFFINE_SILU, ops.PRO_LRELU):
            built = mode == ops.PRO_AFFINE_SILU or (mode == ops.PRO_NONE and not skip)
            assert ops.conv_prec_supported(xv, Cout, mode, ops.PREC_FP8X, skip=skip) == (big and built), (B, H, W, Cin, Cout, skip, mode)
            assert not ops.conv_prec_supported(xv, Cout, mode, ops.PREC_FP8X, skip=skip, sub2=True)
            assert ops.conv_prec_supported(xv, Cout, mode, ops.PREC_16X1, skip=skip) == (not skip or mode == ops.PRO_AFFINE_SILU)
            assert ops.conv_prec_supported(xv, Cout, mode, ops.PREC_16X3, skip=skip)


def test_query_refuses_what_is_not_a_3x3_launch():
    import mudiff_hip
    lib = _lib()
    a = mudiff_hip.ConvArgs()
    a.B, a.H, a.W, a.Cin, a.Cout, a.ks, a.stride, a.pad = 128, 11, 35, 20, 60, 3, 1, 1
    assert lib.mud_conv2d_mfma_tile(C.byref(a)) == mudiff_hip.TILE_8X1R
    assert lib.mud_conv2d_mfma_tile(None) == -1
    for field, bad in (('ks', 1), ('ks', 5), ('B', 0), ('H', 0), ('W', -3), ('Cin', 0), ('Cout', 0)):
        b = mudiff_hip.ConvArgs()
        C.memmove(C.byref(b), C.byref(a), C.sizeof(a))
        setattr(b, field, bad)
        assert lib.mud_conv2d_mfma_tile(C.byref(b)) == -1, (field, bad)


def test_in_up2_and_in_s2d_launches_answer_at_the_size_they_run_at():
    """in_up2: the launch runs at twice the view's size; in_s2d: at half of it with four times the channels.  Both forms are built for 8X2
    and MT1 (in_s2d: under the two fp16 plans only): any other tile, or plan, answers -1 - as the *_supported queries answer 0."""
    import mudiff_hip
    from mudiff_hip import ops
    _lib()
    S = ops.PRO_AFFINE_SILU
    # in_up2, low-resolution view [B, 64, 64, 96] -> the launch is 4 x 128 x 128 x 96 -> 128: 8X2 (the table's row); B = 1: 64 < 256 -> MT1
    assert ops.conv_tile(_view(4, 64, 64, 96), 128, in_up2=True, pro_mode=S) == mudiff_hip.TILE_8X2
    assert ops.conv_tile(_view(4, 64, 64, 96), 128, in_up2=True, pro_mode=S, prec=ops.PREC_FP8X) == mudiff_hip.TILE_8X2
    assert ops.conv_tile(_view(4, 64, 64, 96), 128) == mudiff_hip.TILE_MT1            # (the same view without the up-sampling: 64 workgroups)
    assert ops.conv_tile(_view(1, 64, 64, 96), 128, in_up2=True, pro_mode=S) == mudiff_hip.TILE_MT1
    assert ops.conv_tile(_view(1, 64, 64, 96), 128, in_up2=True, pro_mode=S, prec=ops.PREC_FP8X) == -1      # no MT1 under that plan
    # 2 x 256 x 256 x 80 -> 64 is 16X1 (the table's row): no in_up2 there
    assert ops.conv_tile(_view(2, 128, 128, 80), 64, in_up2=True, pro_mode=S) == -1 and not ops.in_up2_ok(2, 256, 256, 80, 64)
    assert ops.in_up2_ok(4, 128, 128, 96, 128) and ops.in_up2_ok(4, 128, 128, 96, 128, ops.PREC_FP8X)
    # in_s2d, full-resolution view [B, 256, 256, 16] -> folded [B, 128, 128, 64] -> 128: B = 4 is 8X2, B = 1 is MT1
    assert ops.conv_tile(_view(4, 256, 256, 16), 128, in_s2d=True) == mudiff_hip.TILE_8X2 and ops.in_s2d_ok(4, 256, 256, 16, 128)
    assert ops.conv_tile(_view(1, 256, 256, 16), 128, in_s2d=True) == mudiff_hip.TILE_MT1 and ops.in_s2d_ok(1, 256, 256, 16, 128)
    assert ops.conv_tile(_view(4, 256, 256, 16), 128, in_s2d=True, prec=ops.PREC_FP8X) == -1
    # folded [8, 128, 128, 64] -> 64 is 8X1R (4 * 16 * 1 * 8 = 512): not built
    assert ops.conv_tile(_view(8, 256, 256, 16), 64, in_s2d=True) == -1 and not ops.in_s2d_ok(8, 256, 256, 16, 64)


def test_split_k_workspace_is_sized_for_the_tile_the_query_names():
    """mud_conv2d_mfma_splitk_bytes takes the tile from the same function: a small grid with a long reduction is MT1 (256 threads x 32
    accumulators per slab tile), with the fused skip conv twice that - and only with arrival counters."""
    import mudiff_hip
    lib = _lib()
    buf = torch.empty(64)
    a = mudiff_hip.ConvArgs()
    a.x = a.out = C.c_void_p(buf.data_ptr())
    a.B, a.H, a.W, a.Cin, a.ldx, a.ks, a.stride, a.pad, a.Cout, a.ldo = 1, 13, 35, 260, 260, 3, 1, 1, 68, 68
    assert lib.mud_conv2d_mfma_tile(C.byref(a)) == mudiff_hip.TILE_MT1
    blocks = 2 * 4 * 2 * 1                       # column tiles x groups of 4 rows x 64-channel tiles x B
    # 17 chunks of 16 channels over a 16-workgroup grid: four slices (at most 4, at least 4 chunks each)
    assert lib.mud_conv2d_mfma_splitk_bytes(C.byref(a)) == 4 * blocks * 256 * 32 * 4
    a.skip_w, a.pro_mode = C.c_void_p(buf.data_ptr()), mudiff_hip.PRO_AFFINE_SILU
    assert lib.mud_conv2d_mfma_splitk_bytes(C.byref(a)) == 0                     # no arrival counters: the fused launch is not split
    a.splitk_counters, a.splitk_ncounters = C.c_void_p(buf.data_ptr()), 16
    assert lib.mud_conv2d_mfma_splitk_bytes(C.byref(a)) == 2 * 4 * blocks * 256 * 32 * 4


def test_the_in_up2_and_in_s2d_keys_are_no_prologue_modes():
    """MUD_PRO_UP2_AFFINE_SILU (4) and MUD_PRO_S2D (5) key kernels inside the library and are no values of mud_conv_args.pro_mode: the
    plan query says no to them, as to any other unknown mode, on the tiles those kernels exist for (8X2, MT1) and on one they do not."""
    import mudiff_hip
    from mudiff_hip import ops
    lib = _lib()
    for (B, H, W, Cin, Cout), tile in (((4, 128, 128, 96, 128), T8X2), ((1, 20, 37, 48, 96), MT1), ((128, 11, 35, 20, 60), T8X1R)):
        assert ops.conv_tile(_view(B, H, W, Cin), Cout) == _code(tile)
        for mode in (-7, 4, 5, 6, 1 << 30):
            for prec in (mudiff_hip.PREC_16X1, mudiff_hip.PREC_FP8X):
                assert lib.mud_conv2d_mfma_prec_supported(ops._query_args(B, H, W, Cin, Cin, Cout, pro_mode=mode), prec) == 0, (tile, mode, prec)
