"""mud_conv_args.res_up2: a 3x3 matrix-core convolution that forms its residual from the LOW-resolution tensor while loading it
(the x2 FIR up-sampling of the up-sampling residual blocks' skip path, backbones/layerspp.py) - against fp64, next to today's two
launches (ops.fir_nhwc, then `res`), and the launches that must refuse it."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'


def g(t):
    return t.to(DEV)


def _up_fir_fp64(lo, k2d):
    """upfirdn2d(up 2, pad (2, 1)) of lo [B,C,h,w] in fp64: zero-stuff, pad, correlate with the flipped kernel."""
    B, Cc, h, w = lo.shape
    u = torch.zeros(B * Cc, 1, 2 * h, 2 * w, dtype=torch.float64)
    u[:, 0, ::2, ::2] = lo.double().reshape(B * Cc, h, w)
    u = F.pad(u, (2, 1, 2, 1))
    k = torch.from_numpy(np.asarray(k2d, dtype=np.float64)).flip(0, 1)[None, None]
    return F.conv2d(u, k).reshape(B, Cc, 2 * h, 2 * w)


def _problem(B, Ho, Wo, Cc, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cc, Ho, Wo, generator=gen)
    w = torch.randn(Cc, Cc, 3, 3, generator=gen) / math.sqrt(Cc * 9)
    bias = torch.randn(Cc, generator=gen)
    sc, sh = torch.rand(B, Cc, generator=gen) + 0.5, torch.randn(B, Cc, generator=gen)
    lo = torch.randn(B, Cc, Ho // 2, Wo // 2, generator=gen)
    return x, w, bias, sc, sh, lo


def _wide_view(ops, t_nchw, extra=8, c0=4):
    """NHWC view of t inside a wider buffer (ld > C)."""
    B, Cc, H, W = t_nchw.shape
    wide = torch.zeros(B, H, W, Cc + extra, device=DEV)
    wide[..., c0:c0 + Cc] = g(t_nchw).permute(0, 2, 3, 1)
    return ops.View(wide, B, H, W, Cc + extra).slice(c0, Cc)


def _both_paths(B, Ho, Wo, Cc, plans):
    from backbones import up_or_down_sampling
    from mudiff_hip import ops
    kk, up, down, pad = up_or_down_sampling.fir_params('up', (1, 3, 3, 1))
    taps = ops.up2_taps(kk, up, down, pad)
    assert taps == (0.25, 0.75, 0.75, 0.25)
    x, w, bias, sc, sh, lo = _problem(B, Ho, Wo, Cc, seed=Cc + 7 * Ho + Wo)
    a = F.silu(x.double() * sc.double()[:, :, None, None] + sh.double()[:, :, None, None])
    ref = (F.conv2d(a, w.double(), bias.double(), padding=1) + _up_fir_fp64(lo, kk)) * ops.INV_SQRT2
    xv, lov = ops.View.from_nchw(g(x)), _wide_view(ops, lo)
    assert lov.ld > Cc
    kw = dict(mfma=True, pro=(g(sc), g(sh), ops.PRO_AFFINE_SILU), bias=g(bias), out_scale=ops.INV_SQRT2)
    ran = []
    for prec in plans:
        if prec != ops.PREC_16X3 and not ops.conv_prec_supported(xv, Cc, ops.PRO_AFFINE_SILU, prec):
            continue                            # the library has no such plan for this launch
        we = ops.fp8x_weight_exponent(w) if prec == ops.PREC_FP8X else 0
        wp = ops.pack_conv_weight(g(w), prec=prec, w_exp=we)
        hi, _ = ops.fir_nhwc(lov, kk, up, down, pad)                                 # today's path: the skip tensor at full resolution
        # today's path twice: as ops.conv launches it, and unsplit.  A res_up2 launch is never split over K, and the 256-channel
        # cases are small grids with a long reduction, which ops.conv deals to several workgroups (res_up2_ok says no there and
        # the blocks keep their FIR launch): another summation order, whose error differs by more than the residual's roundings
        y_today = ops.conv(xv, wp, 3, Cc, res=hi, prec=prec, w_exp=we, **kw).to_nchw().cpu().double()
        y_unsplit = ops.conv(xv, wp, 3, Cc, res=hi, prec=prec, w_exp=we, split_k=False, **kw).to_nchw().cpu().double()
        y_new = ops.conv(xv, wp, 3, Cc, res=lov, res_up2=taps, prec=prec, w_exp=we, **kw).to_nchw().cpu().double()
        e_today, e_new = float((y_today - ref).abs().max()), float((y_new - ref).abs().max())
        split = not torch.equal(y_today, y_unsplit)
        print(f'res_up2 {B}x{Ho}x{Wo} C={Cc} plan {prec}: max-abs vs fp64 {e_new:.3e}; fir_nhwc + res as ops.conv launches it '
              f'({"split over K" if split else "unsplit"}): {e_today:.3e}')
        assert bool(torch.isfinite(y_new).all())
        # the residual is formed term for term as k_fir_up2_quad forms it: the same bits as the unsplit launch of today's path
        assert torch.equal(y_new, y_unsplit)
        if ops.res_up2_ok(B, Ho, Wo, Cc, Cc):   # where the blocks use it: against today's path as it runs
            assert not split and e_new <= 1.1 * e_today + 1e-7
        ran.append(prec)
    return ran


@pytest.mark.parametrize('Ho,Wo', [(2, 2), (6, 10), (16, 32), (18, 34)])
@pytest.mark.parametrize('Cc', [64, 128, 256])
def test_res_up2_vs_fp64_next_to_the_fir_launch(Cc, Ho, Wo):
    """AdaGN + SiLU prologue, out_scale 1/sqrt(2), B = 2, the low-resolution residual inside a wider buffer: 2x2, 6x10, exactly one
    tile (16x32) and a ragged grid crossing tile borders both ways (18x34); 64 / 128 / 256 channels (one-row and two-row tiles).
    fp16 x 3 always; the fp8 cross-term plan where the library reports it for the launch (these grids are too small for it: the
    chip-filling cases below run it).  ops.conv hands a res_up2 launch no split-K workspace, so the 256-channel cases (small grid,
    long reduction) run unsplit."""
    from mudiff_hip import ops
    assert ops.PREC_16X3 in _both_paths(2, Ho, Wo, Cc, (ops.PREC_16X3, ops.PREC_FP8X))


@pytest.mark.parametrize('B,Ho,Wo,Cc', [(8, 128, 128, 64), (4, 128, 128, 128)])
def test_res_up2_on_the_chip_filling_tiles_under_both_plans(B, Ho, Wo, Cc):
    """The 8-wave tiles of the bench shapes (one-row 8 x 32 px x 64 ch; 8 x 32 px x 128 ch), where MUD_PREC_FP8X is built: same
    comparison under fp16 x 3 and the fp8 cross-term plan."""
    from mudiff_hip import ops
    assert ops.res_up2_ok(B, Ho, Wo, Cc, Cc)
    assert _both_paths(B, Ho, Wo, Cc, (ops.PREC_16X3, ops.PREC_FP8X)) == [ops.PREC_16X3, ops.PREC_FP8X]


def test_res_up2_is_refused_where_it_is_not_built():
    """The 1x1 kernel, sub2, odd H, a prologue it is not built for, the direct convolution and a grid split over K: an error and
    an untouched output, never a result computed some other way."""
    import mudiff_hip
    from mudiff_hip import ops
    lib = mudiff_hip.load()
    keep = []

    def args(B, H, W, Cc, ks, res_hw, sub2=0, pro=2):          # pro 2 = MUD_PRO_AFFINE_SILU
        x = torch.randn(B, H, W, Cc, device=DEV)
        w = torch.randn(Cc, Cc, ks, ks, device=DEV) / math.sqrt(Cc * ks * ks)
        res = torch.randn(B, res_hw[0], res_hw[1], Cc, device=DEV)
        Ho, Wo = (H // 2, W // 2) if sub2 else (H, W)
        out = torch.full((B, Ho, Wo, Cc), 7.0, device=DEV)
        wp = ops.pack_conv_weight(w)
        keep.extend([x, res, wp])
        a = mudiff_hip.ConvArgs()
        a.x, a.B, a.H, a.W, a.Cin, a.ldx = C.c_void_p(x.data_ptr()), B, H, W, Cc, Cc
        a.w, a.ks, a.stride, a.pad, a.sub2 = C.c_void_p(wp.data_ptr()), ks, 1, ks // 2, sub2
        a.res, a.ldr, a.out_scale = C.c_void_p(res.data_ptr()), Cc, 1.0
        a.out, a.Cout, a.ldo = C.c_void_p(out.data_ptr()), Cc, Cc
        a.res_up2, a.res_k = 1, (C.c_float * 4)(0.25, 0.75, 0.75, 0.25)
        sc, sh = torch.ones(B, Cc, device=DEV), torch.zeros(B, Cc, device=DEV)
        keep.extend([sc, sh])
        a.pro_scale, a.pro_shift, a.pro_ld, a.pro_mode = C.c_void_p(sc.data_ptr()), C.c_void_p(sh.data_ptr()), Cc, pro
        return a, out

    def refused(a, out, fn=None, match=b'res_up2'):
        assert (fn or lib.mud_conv2d_mfma)(C.byref(a), mudiff_hip.stream_ptr()) != 0
        assert match in lib.mud_last_error(), lib.mud_last_error()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())

    a, out = args(2, 8, 8, 64, 1, (4, 4))               # the 1x1 kernel
    refused(a, out)
    assert not lib.mud_conv2d_mfma_res_up2_supported(C.byref(a))
    a, out = args(2, 9, 9, 64, 3, (2, 2), sub2=1)       # sub2 (odd H and W by its own contract)
    refused(a, out)
    assert not lib.mud_conv2d_mfma_res_up2_supported(C.byref(a))
    a, out = args(2, 9, 8, 64, 3, (4, 4))               # odd H
    refused(a, out)
    assert not lib.mud_conv2d_mfma_res_up2_supported(C.byref(a))
    a, out = args(2, 8, 8, 64, 3, (4, 4), pro=0)        # another prologue than the residual blocks' AdaGN + SiLU
    refused(a, out)
    assert not lib.mud_conv2d_mfma_res_up2_supported(C.byref(a))
    a, out = args(2, 8, 8, 64, 3, (4, 4))               # the direct convolution
    a.w = a.x                                           # (refused before any weight is read)
    refused(a, out, fn=lib.mud_conv2d_direct)
    # a small grid with a long reduction is split over K when the caller hands a workspace: refused, and the predicate says so
    a, out = args(1, 64, 64, 256, 3, (32, 32))
    cnt = ops.new_splitk_counters(torch.device(DEV))
    a.splitk_counters, a.splitk_ncounters = C.c_void_p(cnt.data_ptr()), cnt.numel()
    nws = lib.mud_conv2d_mfma_splitk_bytes(C.byref(a))
    assert nws > 0 and not lib.mud_conv2d_mfma_res_up2_supported(C.byref(a)) and not ops.res_up2_ok(1, 64, 64, 256, 256)
    ws = torch.empty(nws, device=DEV, dtype=torch.uint8)
    a.splitk_ws, a.splitk_ws_bytes = C.c_void_p(ws.data_ptr()), nws
    refused(a, out)
    assert int(cnt.abs().sum()) == 0
    # the well-formed launch runs
    a, out = args(2, 8, 8, 64, 3, (4, 4))
    assert lib.mud_conv2d_mfma_res_up2_supported(C.byref(a)) and lib.mud_conv2d_mfma(C.byref(a), mudiff_hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
