"""mud_conv_args.in_up2: a 3x3 matrix-core convolution that reads the LOW-resolution input of an up-sampling residual block and forms
FIR x2 (silu(AdaGN(x))) while it stages its A operand (Conv_0 of backbones/layerspp.py's up blocks) - against fp64, next to today's
two launches (ops.fir_nhwc with the prologue, then a MUD_PRO_NONE convolution), and the launches that must refuse it."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'

# low-resolution sizes (the launch runs at twice that): a ragged tile with all four image borders inside it; 2 x 2 exact tiles of the
# four-wave kind (8 x 2 of the eight-wave kind: 32 x 64), so the low-resolution halo crosses interior tile borders; an odd size
SIZES = [(6, 10), (16, 32), (9, 7)]
# the two tiles the form is built for are reached the way mud_conv2d_mfma itself picks them (cm_variant3's block counts), by the batch
# size: at B = 2 every size takes the four-wave 4 x 32 px x 64 ch tile; the eight-wave 8 x 32 px x 128 ch tile needs 256 workgroups
# and an even number of 64-channel tiles (128 output channels: two channel tiles in one workgroup)
TILES = {'mt1': dict(B=lambda h, w: 2, couts=(64, 128)),
         '8x2': dict(B=lambda h, w: -(-256 // (-(-2 * w // 32) * -(-2 * h // 8))), couts=(128,))}


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


def _fir():
    from backbones import up_or_down_sampling
    from mudiff_hip import ops
    kk, up, down, pad = up_or_down_sampling.fir_params('up', (1, 3, 3, 1))
    taps = ops.up2_taps(kk, up, down, pad)
    assert taps == (0.25, 0.75, 0.75, 0.25)
    return kk, up, down, pad, taps


def _plans(ops, tile):
    return (ops.PREC_16X3, ops.PREC_FP8X, ops.PREC_16X1) if tile == '8x2' else (ops.PREC_16X3, ops.PREC_16X1)


def _out_with_stats(ops, B, H, W, Cc):
    return ops.View(torch.empty(B, H, W, Cc, device=DEV), B, H, W, Cc, stats=torch.zeros(B, Cc, 2, device=DEV, dtype=torch.float64))


def _three_ways(ops, xv, pro, w, bias, b2, Cout, prec, B, h, wd):
    """(a) the single launch, (b) today's two launches, each with the GroupNorm statistics of its output."""
    kk, up, down, pad, taps = _fir()
    we = ops.fp8x_weight_exponent(w) if prec == ops.PREC_FP8X else 0
    wp = ops.pack_conv_weight(g(w), prec=prec, w_exp=we)
    kw = dict(mfma=True, bias=g(bias), bias2=g(b2), prec=prec, w_exp=we)
    assert ops.in_up2_ok(B, 2 * h, 2 * wd, xv.C, Cout, prec), 'the case must be one the form is built for'
    oa, ob = _out_with_stats(ops, B, 2 * h, 2 * wd, Cout), _out_with_stats(ops, B, 2 * h, 2 * wd, Cout)
    ops.conv(xv, wp, 3, Cout, pro=pro, in_up2=taps, out=oa, **kw)
    h_in, _ = ops.fir_nhwc(xv, kk, up, down, pad, pro=pro, want_h=True)
    if prec != ops.PREC_16X3:
        assert ops.conv_prec_supported(h_in, Cout, ops.PRO_NONE, prec)
    ops.conv(h_in, wp, 3, Cout, out=ob, split_k=False, **kw)      # (an in_up2 launch is never split over K)
    return oa, ob


def _check(tag, oa, ob, ref, prec, ops):
    ya, yb = oa.to_nchw().cpu().double(), ob.to_nchw().cpu().double()
    ea, eb = float((ya - ref).abs().max()), float((yb - ref).abs().max())
    print(f'in_up2 {tag} plan {prec}: max-abs vs fp64 {ea:.3e}; fir_nhwc + MUD_PRO_NONE conv {eb:.3e}; bit-identical {torch.equal(ya, yb)}')
    assert bool(torch.isfinite(ya).all())
    # against today's path, measured on the same inputs; the absolute floor is test_conv_fp8x_plan_vs_fp64's
    assert ea <= 1.25 * eb + 1e-6, (tag, prec, ea, eb)
    # the activation is k_fir_up2_quad's prologue, instruction for instruction, and the polyphase sums are its chain: the same bits
    assert torch.equal(ya, yb), (tag, prec)
    # the statistics are per-wave fp32 partial sums of identical stored values over identical tiles, added to fp64 by atomics: only
    # the order of those fp64 additions differs between two launches, <= (number of partials) x 2^-53 of the sum of their magnitudes
    sa, sb = oa.stats.cpu(), ob.stats.cpu()
    scale = float(yb.pow(2).sum(dim=(2, 3)).max()) + 1.0
    assert float((sa - sb).abs().max()) <= 1e-10 * scale, (tag, prec, float((sa - sb).abs().max()), scale)
    # and they are the statistics of what was stored (fp32 partial sums: 2^-24 per addition)
    want = torch.stack([ya.sum(dim=(2, 3)), ya.pow(2).sum(dim=(2, 3))], dim=-1)
    assert float((sa - want).abs().max()) <= 1e-4 * scale


@pytest.mark.parametrize('tile', sorted(TILES))
@pytest.mark.parametrize('Cin', [16, 20, 48])
@pytest.mark.parametrize('h,w', SIZES)
def test_in_up2_vs_fp64_next_to_the_fir_launch(h, w, Cin, tile):
    """One chunk, a partial chunk and three chunks of input channels; one and two 64-channel tiles; scale, shift and time-embedding
    bias different per sample; every plan the tile has the form for.  Each case: error against the fp64 composition (affine, SiLU,
    upfirdn2d x2, conv3x3) within 1.25 x the error of today's two launches on the same inputs + 1e-6, and - the SiLU sequence and the
    polyphase chain being those of k_fir_up2_quad - the same bits as today's two launches; GroupNorm statistics alike."""
    from mudiff_hip import ops
    kk = _fir()[0]
    B = TILES[tile]['B'](h, w)
    for Cout in TILES[tile]['couts']:
        gen = torch.Generator().manual_seed(1000 * h + 10 * Cin + Cout + B)
        x = torch.randn(B, Cin, h, w, generator=gen)
        wt = torch.randn(Cout, Cin, 3, 3, generator=gen) / math.sqrt(Cin * 9)
        bias, b2 = torch.randn(Cout, generator=gen), torch.randn(B, Cout, generator=gen)
        sc, sh = torch.rand(B, Cin, generator=gen) + 0.5, torch.randn(B, Cin, generator=gen)
        act = F.silu(x.double() * sc.double()[:, :, None, None] + sh.double()[:, :, None, None])
        ref = F.conv2d(_up_fir_fp64(act, kk), wt.double(), bias.double(), padding=1) + b2.double()[:, :, None, None]
        xv = ops.View.from_nchw(g(x))
        for prec in _plans(ops, tile):
            oa, ob = _three_ways(ops, xv, (g(sc), g(sh), ops.PRO_AFFINE_SILU), wt, bias, b2, Cout, prec, B, h, w)
            _check(f'{tile} B={B} {h}x{w} {Cin}->{Cout}', oa, ob, ref, prec, ops)


@pytest.mark.parametrize('tile', sorted(TILES))
def test_in_up2_with_the_groupnorm_finalisation_folded_in(tile):
    """The prologue as the blocks hand it over: a LazyGN over the producer's (sum, sumsq) with per-sample gamma / beta, finalised in
    the kernel's prologue with the LOW-resolution pixel count - next to fir_nhwc, which takes the finalised arrays."""
    from mudiff_hip import ops
    kk = _fir()[0]
    h, w, Cin, Cout, G = 16, 32, 48, 128, 12
    B = TILES[tile]['B'](h, w)
    gen = torch.Generator().manual_seed(77 + B)
    x = torch.randn(B, Cin, h, w, generator=gen) * 1.5 + 0.3
    wt = torch.randn(Cout, Cin, 3, 3, generator=gen) / math.sqrt(Cin * 9)
    bias, b2 = torch.randn(Cout, generator=gen), torch.randn(B, Cout, generator=gen)
    gamma, beta = torch.rand(B, Cin, generator=gen) + 0.5, torch.randn(B, Cin, generator=gen)
    xd = x.double()
    xn = F.group_norm(xd, G, eps=1e-6) * gamma.double()[:, :, None, None] + beta.double()[:, :, None, None]
    ref = F.conv2d(_up_fir_fp64(F.silu(xn), kk), wt.double(), bias.double(), padding=1) + b2.double()[:, :, None, None]
    xv = ops.View.from_nchw(g(x))
    xv.stats = g(torch.stack([xd.sum(dim=(2, 3)), xd.pow(2).sum(dim=(2, 3))], dim=-1).contiguous())
    for prec in _plans(ops, tile):
        lazy = ops.gn_lazy(xv, G, g(gamma), g(beta))
        assert isinstance(lazy, ops.LazyGN)
        oa, ob = _three_ways(ops, xv, (lazy, None, ops.PRO_AFFINE_SILU), wt, bias, b2, Cout, prec, B, h, w)
        _check(f'{tile} folded GroupNorm B={B}', oa, ob, ref, prec, ops)


def test_in_up2_is_refused_where_it_is_not_built():
    """sub2, the fused skip conv, a grid split over K, an odd output size, a plan and a tile the form is not built for, the 1x1 kernel
    and the direct convolution: an error and an untouched output, never a result computed some other way."""
    import mudiff_hip
    from mudiff_hip import ops
    lib = mudiff_hip.load()
    keep = []

    def args(B, H, W, Cc, ks=3, sub2=0, prec=0):               # H, W: the launch's (output) size; x is allocated at that size, more than in_up2 reads
        x = torch.randn(B, H, W, Cc, device=DEV)
        w = torch.randn(Cc, Cc, ks, ks, device=DEV) / math.sqrt(Cc * ks * ks)
        Ho, Wo = (H // 2, W // 2) if sub2 else (H, W)
        out = torch.full((B, Ho, Wo, Cc), 7.0, device=DEV)
        we = ops.fp8x_weight_exponent(w) if prec == ops.PREC_FP8X else 0
        wp = ops.pack_conv_weight(w, prec=prec, w_exp=we) if ks == 3 else ops.pack_conv_weight(w)
        sc, sh = torch.ones(B, Cc, device=DEV), torch.zeros(B, Cc, device=DEV)
        keep.extend([x, wp, sc, sh])
        a = mudiff_hip.ConvArgs()
        a.x, a.B, a.H, a.W, a.Cin, a.ldx = C.c_void_p(x.data_ptr()), B, H, W, Cc, Cc
        a.w, a.ks, a.stride, a.pad, a.sub2, a.out_scale = C.c_void_p(wp.data_ptr()), ks, 1, ks // 2, sub2, 1.0
        a.out, a.Cout, a.ldo, a.prec, a.w_exp = C.c_void_p(out.data_ptr()), Cc, Cc, prec, we
        a.in_up2, a.in_k = 1, (C.c_float * 4)(0.25, 0.75, 0.75, 0.25)
        a.pro_scale, a.pro_shift, a.pro_ld, a.pro_mode = C.c_void_p(sc.data_ptr()), C.c_void_p(sh.data_ptr()), Cc, ops.PRO_AFFINE_SILU
        return a, out

    def refused(a, out, fn=None):
        assert not lib.mud_conv2d_mfma_in_up2_supported(C.byref(a))
        assert (fn or lib.mud_conv2d_mfma)(C.byref(a), mudiff_hip.stream_ptr()) != 0
        assert b'in_up2' in lib.mud_last_error(), lib.mud_last_error()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())

    refused(*args(2, 9, 9, 64, sub2=1))                 # sub2 (odd H and W by its own contract)
    a, out = args(2, 8, 8, 64)                          # the fused skip conv
    so = torch.full((2, 8, 8, 64), 7.0, device=DEV)
    sw = ops.pack_conv_weight(torch.randn(64, 64, 1, 1, device=DEV))
    keep.extend([so, sw])
    a.skip_w, a.skip_out, a.skip_ldo = C.c_void_p(sw.data_ptr()), C.c_void_p(so.data_ptr()), 64
    refused(a, out)
    assert bool((so == 7.0).all())
    refused(*args(2, 8, 9, 64))                         # odd output width
    refused(*args(2, 9, 8, 64))                         # odd output height
    refused(*args(2, 8, 8, 64, prec=ops.PREC_FP8X))     # a plan that is not built for the launch's tile
    a, out = args(128, 32, 32, 64)                      # a tile the form is not built for (one 64-channel tile on eight waves)
    assert not ops.in_up2_ok(128, 32, 32, 64, 64)
    refused(a, out)
    refused(*args(2, 8, 8, 64, ks=1))                   # the 1x1 kernel
    a, out = args(2, 8, 8, 64)                          # the direct convolution
    a.w = a.x                                           # (refused before any weight is read)
    assert lib.mud_conv2d_direct(C.byref(a), mudiff_hip.stream_ptr()) != 0 and b'in_up2' in lib.mud_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # a small grid with a long reduction is split over K when the caller hands a workspace: refused, and the predicate says so
    a, out = args(1, 64, 64, 256)
    cnt = ops.new_splitk_counters(torch.device(DEV))
    a.splitk_counters, a.splitk_ncounters = C.c_void_p(cnt.data_ptr()), cnt.numel()
    nws = lib.mud_conv2d_mfma_splitk_bytes(C.byref(a))
    assert nws > 0 and not ops.in_up2_ok(1, 64, 64, 256, 256)
    ws = torch.empty(nws, device=DEV, dtype=torch.uint8)
    a.splitk_ws, a.splitk_ws_bytes = C.c_void_p(ws.data_ptr()), nws
    refused(a, out)
    assert int(cnt.abs().sum()) == 0
    # the well-formed launch runs
    a, out = args(2, 8, 8, 64)
    assert lib.mud_conv2d_mfma_in_up2_supported(C.byref(a)) and lib.mud_conv2d_mfma(C.byref(a), mudiff_hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


def test_a_filter_up2_taps_rejects_keeps_the_fir_launch(monkeypatch):
    """An up block whose up-sampler is not the separable 4x4 filter (fir=False: nearest-neighbour repeat) launches the same kernels
    with the switch on and off; the FIR block drops exactly one fir_nhwc launch (RES_UP2 off: only Conv_0's changes)."""
    from backbones import layerspp, up_or_down_sampling
    from mudiff_hip import ops
    assert ops.up2_taps(*up_or_down_sampling.fir_params('naive_up', (1, 3, 3, 1))) is None
    monkeypatch.setattr(ops, 'RES_UP2', False)
    gen = torch.Generator().manual_seed(3)
    x, zemb = g(torch.randn(2, 32, 8, 8, generator=gen)), g(torch.randn(2, 64, generator=gen))
    counts, outs = {}, {}
    for fir in (False, True):
        torch.manual_seed(11)
        blk = layerspp.ResnetBlockBigGANpp_Adagn(torch.nn.SiLU(), 32, 32, temb_dim=None, zemb_dim=64, up=True, fir=fir, init_scale=1.0).to(DEV).eval()
        assert blk.prepared()['c0'].mfma
        for on in (True, False):
            monkeypatch.setattr(ops, 'IN_UP2', on)
            ops.PROFILE.enable()
            outs[fir, on] = blk(x, zemb=zemb)
            counts[fir, on] = {k: v['n'] for k, v in ops.PROFILE.summary().items()}
            ops.PROFILE.disable()
    assert counts[False, True] == counts[False, False] and torch.equal(outs[False, True], outs[False, False])
    assert counts[True, False]['fir_nhwc'] - counts[True, True]['fir_nhwc'] == 1, (counts[True, False], counts[True, True])
    assert float((outs[True, True] - outs[True, False]).abs().max()) <= 1e-5
