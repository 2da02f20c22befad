"""mud_conv_args.in_s2d: a 3x3 matrix-core convolution over the 2x2 space-to-depth view of its input, gathered from the
full-resolution tensor while the A operand is staged - the input pyramid's FIR + stride-2 conv as ONE launch.
Addressing against a materialised fold (same bits), the launches that must refuse the flag, and the folded down-sampler against fp64
next to today's two launches."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'

# the two tiles the form is built for are reached the way mud_conv2d_mfma itself picks them (cm_variant3's block counts), by the batch
# size: at B = 2 every size below takes the four-wave 4 x 32 px x 64 ch tile; the eight-wave 8 x 32 px x 128 ch tile needs 256
# workgroups of 8 x 32 VIEW pixels and an even number of 64-channel tiles (128 output channels)
TILES = {'mt1': dict(B=lambda h, w: 2, couts=(64, 128)),
         '8x2': dict(B=lambda h, w: -(-256 // (-(-(w // 2) // 32) * -(-(h // 2) // 8))), couts=(128,))}
# size of x, channels, (ld, c0) of the buffer x is a slice of: one 16-channel chunk per parity on exactly one 8 x 32 view tile;
# view 12 x 40 - tile rows and columns that do not divide, two view tiles along each axis, two chunks per parity; the same as a
# 32-channel slice at offset 16 of a 64-channel buffer (ldx != C)
CASES = {'16x64-c16': (16, 64, 16, None), '24x80-c32': (24, 80, 32, None), '24x80-c32-slice': (24, 80, 32, (64, 16))}


def g(t):
    return t.to(DEV)


@pytest.mark.parametrize('tile', sorted(TILES))
@pytest.mark.parametrize('case', sorted(CASES))
def test_in_s2d_stages_the_bits_of_a_materialised_fold(case, tile):
    """The flag changes staging ADDRESSES only: on the same packed weights the launch on x equals, bit for bit, the plain launch on
    ops.s2d_fold(x), under both fp16 plans, with and without a residual and an output scale (B = 2 on the four-wave tile)."""
    from mudiff_hip import ops
    H, W, Cc, sl = CASES[case]
    B = TILES[tile]['B'](H, W)
    ld, c0 = sl if sl else (Cc, 0)
    for Cout in TILES[tile]['couts']:
        gen = torch.Generator().manual_seed(H * 100 + Cc + Cout + B)
        base = g(torch.randn(B, H, W, ld, generator=gen))
        xv = ops.View(base, B, H, W, Cc, ld, c0)
        fv = ops.View(ops.s2d_fold(xv.tensor()), B, H // 2, W // 2, 4 * Cc)
        assert torch.equal(fv.tensor()[:, 1, 2, 2 * Cc + 3], xv.tensor()[:, 3, 4, 3])          # parity (1, 0) of view pixel (1, 2) is pixel (3, 4)
        w = torch.randn(Cout, 4 * Cc, 3, 3, generator=gen) / math.sqrt(36 * Cc)
        bias = g(torch.randn(Cout, generator=gen))
        res = ops.View(g(torch.randn(B, H // 2, W // 2, Cout, generator=gen)), B, H // 2, W // 2, Cout)
        for prec in (ops.PREC_16X3, ops.PREC_16X1):
            assert ops.in_s2d_ok(B, H, W, Cc, Cout, prec), 'the case must be one the form is built for'
            wp = ops.pack_conv_weight(g(w), prec=prec)
            for kw in (dict(), dict(res=res, out_scale=0.7)):
                oa = ops.conv(xv, wp, 3, Cout, mfma=True, bias=bias, prec=prec, in_s2d=True, **kw)
                ob = ops.conv(fv, wp, 3, Cout, mfma=True, bias=bias, prec=prec, split_k=False, **kw)      # (an in_s2d launch is never split over K)
                ya, yb = oa.tensor(), ob.tensor()
                assert ya.shape == (B, H // 2, W // 2, Cout) and bool(torch.isfinite(ya).all()) and float(ya.abs().max()) > 0.1
                assert torch.equal(ya, yb), (case, tile, Cout, prec, sorted(kw), float((ya - yb).abs().max()))


def test_in_s2d_is_refused_where_it_is_not_built():
    """24 channels (a chunk would straddle two parities), sub2, the fused skip conv, a prologue, the fp8 plan, a tile the form is not built
    for, the 1x1 kernel, the direct convolution and a grid split over K: the ABI's error and an untouched output, never a result
    computed some other way.  An odd full-resolution size cannot be written into the argument struct (H and W are the view's, x is
    [B, 2H, 2W, Cin/4]): ops.conv refuses it before anything is launched."""
    import mudiff_hip
    from mudiff_hip import ops
    lib = mudiff_hip.load()
    keep = []

    def args(B, Hv, Wv, Cc, Cout=64, ks=3, sub2=0, prec=0, pro=0):      # Hv, Wv: the view's size; x is allocated as [B, 2Hv, 2Wv, Cc]
        x = torch.randn(B, 2 * Hv, 2 * Wv, Cc, device=DEV)
        w = torch.randn(Cout, 4 * Cc, ks, ks, device=DEV) / math.sqrt(4 * Cc * ks * ks)
        Ho, Wo = (Hv // 2, Wv // 2) if sub2 else (Hv, Wv)
        out = torch.full((B, Ho, Wo, Cout), 7.0, device=DEV)
        we = ops.fp8x_weight_exponent(w) if prec == ops.PREC_FP8X else 0
        wp = ops.pack_conv_weight(w, prec=prec, w_exp=we) if ks == 3 else ops.pack_conv_weight(w)
        sc, sh = torch.ones(B, 4 * Cc, device=DEV), torch.zeros(B, 4 * Cc, device=DEV)
        keep.extend([x, wp, sc, sh])
        a = mudiff_hip.ConvArgs()
        a.x, a.B, a.H, a.W, a.Cin, a.ldx = C.c_void_p(x.data_ptr()), B, Hv, Wv, 4 * Cc, Cc
        a.w, a.ks, a.stride, a.pad, a.sub2, a.out_scale = C.c_void_p(wp.data_ptr()), ks, 1, ks // 2, sub2, 1.0
        a.out, a.Cout, a.ldo, a.prec, a.w_exp = C.c_void_p(out.data_ptr()), Cout, Cout, prec, we
        a.in_s2d, a.pro_mode = 1, pro
        if pro:
            a.pro_scale, a.pro_shift, a.pro_ld = C.c_void_p(sc.data_ptr()), C.c_void_p(sh.data_ptr()), 4 * Cc
        return a, out

    def refused(a, out, fn=None):
        assert not lib.mud_conv2d_mfma_in_s2d_supported(C.byref(a))
        assert (fn or lib.mud_conv2d_mfma)(C.byref(a), mudiff_hip.stream_ptr()) != 0
        assert b'in_s2d' in lib.mud_last_error(), lib.mud_last_error()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())

    refused(*args(2, 8, 8, 24))                          # C = 24: Cin = 96 is no multiple of 64
    assert not ops.in_s2d_ok(2, 16, 16, 24, 64)
    refused(*args(2, 9, 9, 16, sub2=1))                  # sub2 (odd H and W by its own contract)
    a, out = args(2, 8, 8, 16)                           # the fused skip conv
    so = torch.full((2, 8, 8, 64), 7.0, device=DEV)
    sw = ops.pack_conv_weight(torch.randn(64, 64, 1, 1, device=DEV))
    keep.extend([so, sw])
    a.skip_w, a.skip_out, a.skip_ldo = C.c_void_p(sw.data_ptr()), C.c_void_p(so.data_ptr()), 64
    refused(a, out)
    assert bool((so == 7.0).all())
    refused(*args(2, 8, 8, 16, pro=ops.PRO_AFFINE_SILU))   # a prologue
    refused(*args(256, 8, 32, 16, Cout=128, prec=ops.PREC_FP8X))      # the fp8 plan (on a tile that plan has)
    a, out = args(128, 32, 32, 16)                       # a tile the form is not built for (one 64-channel tile on eight waves)
    assert not ops.in_s2d_ok(128, 64, 64, 16, 64)
    refused(a, out)
    refused(*args(2, 8, 8, 16, ks=1))                    # the 1x1 kernel
    a, out = args(2, 8, 8, 16)                           # the direct convolution
    a.w = a.x                                            # (refused before any weight is read)
    assert lib.mud_conv2d_direct(C.byref(a), mudiff_hip.stream_ptr()) != 0 and b'in_s2d' in lib.mud_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # a small grid with a long reduction is split over K when the caller hands a workspace: refused, and the predicate says so
    a, out = args(1, 64, 64, 64, Cout=128)
    cnt = ops.new_splitk_counters(torch.device(DEV))
    a.splitk_counters, a.splitk_ncounters = C.c_void_p(cnt.data_ptr()), cnt.numel()
    a.in_s2d = 0
    nws = lib.mud_conv2d_mfma_splitk_bytes(C.byref(a))
    a.in_s2d = 1
    assert nws > 0 and not ops.in_s2d_ok(1, 128, 128, 64, 128)
    ws = torch.empty(nws, device=DEV, dtype=torch.uint8)
    a.splitk_ws, a.splitk_ws_bytes = C.c_void_p(ws.data_ptr()), nws
    refused(a, out)
    assert int(cnt.abs().sum()) == 0
    # an odd full-resolution height or width: no argument struct describes it; ops.conv raises before it builds one
    for hw in ((15, 16), (16, 15)):
        xo = ops.View(torch.randn(2, *hw, 16, device=DEV), 2, *hw, 16)
        assert not ops.in_s2d_ok(2, *hw, 16, 64)
        with pytest.raises(mudiff_hip.MudiffHipError, match='in_s2d'):
            ops.conv(xo, keep[1], 3, 64, mfma=True, in_s2d=True)
    # the well-formed launch runs
    a, out = args(2, 8, 8, 16)
    assert lib.mud_conv2d_mfma_in_s2d_supported(C.byref(a)) and lib.mud_conv2d_mfma(C.byref(a), mudiff_hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


def _fir_then_conv_fp64(x, w, k1d):
    B, Cc, H, W = x.shape
    k2 = torch.from_numpy(np.outer(k1d, k1d)).double().flip(0, 1)[None, None]
    xf = F.conv2d(F.pad(x.double(), (2, 2, 2, 2)).reshape(B * Cc, 1, H + 4, W + 4), k2).reshape(B, Cc, H + 1, W + 1)
    return F.conv2d(xf, w.double(), stride=2)


# what the folded launch's max-abs error was MEASURED to exceed the two launches' by on these cases (MI355X; seeded inputs, no atomics in
# either path: the figures repeat), times two.  (tile, weight scale, residual) -> allowed excess; 0 where the folded launch was the
# more exact one.  Recorded (a) | (b): see the docstring below.
EXCESS = {('mt1', 1.0, False): 2.2e-6, ('mt1', 37.0, False): 3.8e-5, ('mt1', 1.0 / 512, False): 0.0,
          ('mt1', 1.0, True): 6.4e-6, ('mt1', 37.0, True): 2.8e-5, ('mt1', 1.0 / 512, True): 4.4e-6,
          ('8x2', 1.0, False): 1.1e-6, ('8x2', 37.0, False): 5.7e-5, ('8x2', 1.0 / 512, False): 0.0,
          ('8x2', 1.0, True): 6.9e-6, ('8x2', 37.0, True): 3.8e-5, ('8x2', 1.0 / 512, True): 4.0e-6}


@pytest.mark.parametrize('tile,B,H,W,Cc,Cout', [('mt1', 2, 64, 64, 32, 128), ('8x2', 256, 16, 64, 16, 128)])
def test_folded_downsampler_vs_fp64_next_to_the_two_launches(tile, B, H, W, Cc, Cout, monkeypatch):
    """Conv2d(down=True) with the switch on (b) and off (a), both against the fp64 composition FIR-then-conv on the CPU, at the
    weight scales of test_conv_fp8x_plan_vs_fp64 (x1, x37, /512); once with the bias alone and once as the generators run it (bias,
    residual, 1/sqrt(2)).

    Max-abs: (b) may exceed (a) by at most twice what was measured for the case (EXCESS).
    Rms: (b) stays below ONE TENTH of what that test grants the fp8 plan per launch, with or without a residual (4e-5 of the
    convolution's rms + 1e-6): 4e-6 * rms + 1e-7, rms = that of the convolution as it reaches the output (times out_scale).  With a
    residual one allowance is added, for the one thing the folded launch does that the sub2 launch does not: like every other 3x3
    launch with a residual it accumulates ON TOP of it (the sub2 launch adds it in the epilogue), so each of its N = 3 K / 16
    accumulations (three MFMAs per 16-channel tap, K = 36 C products) rounds a number of the residual's size to fp32.  One such
    rounding has an rms of at most 2^-23 / sqrt(12) of the value (uniform in half an ulp, the ulp at most 2^-23 of the value); N
    independent ones add in quadrature: sqrt(N) * 2^-23 / sqrt(12) * rms(residual) * out_scale = 3.6e-7 (C = 32) and 2.5e-7 (C = 16)
    for the unit-size residual here.  Nothing about the convolution's own error is allowed for.
    The pre-scale of the operand (fold_weight_exponent) is what keeps the /512 case inside the rms bar: without it the composed taps
    (down to 1/64 of a weight) are fp16 subnormals and the error is absolute, 2^-25 per tap.
    Measured on MI355X, max-abs (a) | (b) at x1, x37, /512.  Bias alone - four-wave tile: 7.2e-7 | 1.8e-6, 2.5e-5 | 4.4e-5, 4.6e-7 | 2.5e-9;
    eight-wave tile: 7.6e-7 | 1.3e-6, 2.2e-5 | 5.0e-5, 3.5e-7 | 2.2e-9; rms (b) 1.2e-7, 4.4e-6, 2.3e-10 and 8.6e-8, 3.2e-6, 1.7e-10 against
    bars of 1.3e-6, 4.6e-5, 1.0e-7.  With the residual - 5.1e-7 | 3.7e-6, 1.9e-5 | 3.3e-5, 3.5e-7 | 2.5e-6 and 6.2e-7 | 4.1e-6, 1.8e-5 | 3.7e-5,
    3.7e-7 | 2.4e-6; rms (b) 3.8e-7, 3.2e-6, 2.3e-7 and 2.6e-7, 2.4e-6, 1.7e-7 against bars of 1.3e-6, 3.3e-5, 4.6e-7 and 1.2e-6, 3.2e-5, 3.5e-7."""
    from backbones import up_or_down_sampling as ud
    from mudiff_hip import ops
    assert ops.in_s2d_ok(B, H, W, Cc, Cout)
    t = ud.separable_taps(*[ud.fir_params('conv_down', (1, 3, 3, 1), conv_k=3)[i] for i in (0, 3)])
    gen = torch.Generator().manual_seed(B + H + Cc)
    rms = lambda e: float(e.pow(2).mean().sqrt())      # noqa: E731
    for wscale in (1.0, 37.0, 1.0 / 512):
        x = torch.randn(B, Cc, H, W, generator=gen)
        w = torch.randn(Cout, Cc, 3, 3, generator=gen) / math.sqrt(9 * Cc) * wscale
        bias, r = torch.randn(Cout, generator=gen) * wscale, torch.randn(B, Cout, H // 2, W // 2, generator=gen)
        conv = _fir_then_conv_fp64(x, w, t)
        m = ud.Conv2d(Cc, Cout, 3, down=True).to(DEV)
        m.weight.data.copy_(w)
        m.bias.data.copy_(bias)
        xv, rv = ops.View.from_nchw(g(x)), ops.View.from_nchw(g(r))
        for with_res in (False, True):
            osc = 1.0 / math.sqrt(2.0) if with_res else 1.0
            ref = (conv + bias.double()[None, :, None, None] + (r.double() if with_res else 0.0)) * osc
            outs = {}
            for on in (False, True):
                monkeypatch.setattr(ops, 'PYR_S2D', on)
                ops.PROFILE.enable()
                outs[on] = m.run(xv, res=rv if with_res else None, out_scale=osc).to_nchw().cpu().double()
                names = {k: v['n'] for k, v in ops.PROFILE.summary().items() if k != 'pack_weights'}      # (the operands are packed on first use)
                ops.PROFILE.disable()
                assert names == ({'conv_mfma_k3': 1} if on else {'fir_nhwc': 1, 'conv_mfma_k3': 1}), names
            ea, eb = float((outs[False] - ref).abs().max()), float((outs[True] - ref).abs().max())
            ra, rb, conv_rms = rms(outs[False] - ref), rms(outs[True] - ref), rms(conv) * osc
            excess = EXCESS[tile, wscale, with_res]
            on_top = math.sqrt(3 * 36 * Cc / 16) * 2.0 ** -23 / math.sqrt(12.0) * rms(r.double()) * osc if with_res else 0.0
            bar = 4e-6 * conv_rms + 1e-7 + on_top
            print(f'pyr_s2d {tile} B={B} {H}x{W} {Cc}->{Cout} w x{wscale:g} (2^{m._folded_weights(ops.PREC_16X3)[1]}) {"bias+res" if with_res else "bias"}: '
                  f'max-abs vs fp64 two launches {ea:.3e} | folded {eb:.3e} (may exceed by {excess:.1e}); rms {ra:.3e} | {rb:.3e}, bar {bar:.3e}'
                  f'{f" (of it {on_top:.2e} for accumulating on the residual)" if with_res else ""}; conv rms {conv_rms:.3g}')
            assert bool(torch.isfinite(outs[True]).all())
            assert eb <= ea + excess, (wscale, with_res, ea, eb, excess)
            assert rb <= bar, (wscale, with_res, rb, bar, conv_rms)


@pytest.mark.parametrize('tile,B', [('mt1', 2), ('8x2', 64)])
def test_in_s2d_weight_prescale_is_exact(tile, B):
    """w_exp: a launch on weights W * 2^e with w_exp = e gives the bits of the plain launch on the fold with W itself.  The residual
    goes into the accumulators times 2^e and the power of two leaves the sum before the epilogue; every fp32 rounding in between
    commutes with a power of two.  The weights are made of fp16 numbers no smaller than 2^-10 in magnitude, so that hi pieces are
    normal and lo pieces zero in both operands (a tap that is subnormal in one of them is what the pre-scale is there to change)."""
    from mudiff_hip import ops
    H, W, Cc, Cout = 24, 80, 32, 128
    gen = torch.Generator().manual_seed(41 + B)
    xv = ops.View(g(torch.randn(B, H, W, Cc, generator=gen)), B, H, W, Cc)
    fv = ops.View(ops.s2d_fold(xv.tensor()), B, H // 2, W // 2, 4 * Cc)
    w = (torch.randn(Cout, 4 * Cc, 3, 3, generator=gen) / math.sqrt(36 * Cc)).half().float()
    w = torch.where(w.abs() < 2.0 ** -10, torch.full_like(w, 2.0 ** -10), w)
    bias = g(torch.randn(Cout, generator=gen))
    res = ops.View(g(torch.randn(B, H // 2, W // 2, Cout, generator=gen)), B, H // 2, W // 2, Cout)
    for prec in (ops.PREC_16X3, ops.PREC_16X1):
        assert ops.in_s2d_ok(B, H, W, Cc, Cout, prec)
        plain = ops.pack_conv_weight(g(w), prec=prec)
        for e in (5, -3):
            scaled = ops.pack_conv_weight(g(w * 2.0 ** e), prec=prec)
            for kw in (dict(), dict(res=res, out_scale=0.7)):
                oa = ops.conv(xv, scaled, 3, Cout, mfma=True, bias=bias, prec=prec, in_s2d=True, w_exp=e, **kw)
                ob = ops.conv(fv, plain, 3, Cout, mfma=True, bias=bias, prec=prec, split_k=False, **kw)
                assert float(oa.tensor().abs().max()) > 0.1
                assert torch.equal(oa.tensor(), ob.tensor()), (tile, prec, e, sorted(kw), float((oa.tensor() - ob.tensor()).abs().max()))
