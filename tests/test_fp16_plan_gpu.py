"""GPU: the single-pass fp16 plan (MUD_PREC_16X1, MUD_PREC_PLAN=fp16).  Every 3x3 tile / prologue / fused-skip / split-K form of the
kernel against an fp64 convolution of its own definition (fp16(prologue(x)) * fp16(w), fp32 accumulation); saturation; the launch
record of G1 + G2 under the plan; the whole sampler against the oracle with the same operands rounded; graph = eager; the driver."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import PKG, REPO
from helpers import SMALL_CFGS, check_fp16_definition as _check, demo_conds, h16 as _h16, load_golden, pro_host as _pro_host, sampler_inputs
from oracle import mudiff_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'


def g(t):
    return t.to(DEV)


# (B, H, W, Cin, Cout, prologue, tile cm_variant3 picks): one shape per tile variant and prologue mode
CASES = [(2, 256, 256, 64, 64, 'none', '8X1R'), (4, 128, 128, 96, 128, 'silu', '8X2'), (2, 256, 256, 80, 64, 'none', '16X1'),
         (64, 8, 256, 68, 64, 'silu', 'MT2'), (1, 20, 37, 48, 96, 'none', 'MT1'), (1, 20, 37, 48, 96, 'affine', 'MT1'),
         (1, 20, 37, 48, 96, 'lrelu', 'MT1'), (1, 20, 37, 48, 96, 'silu', 'MT1'), (2, 33, 70, 32, 64, 'affine', 'MT1')]


@pytest.mark.parametrize('B,H,W,Cin,Cout,pro,tile', CASES)
def test_plain_launch_exact_against_its_definition(B, H, W, Cin, Cout, pro, tile):
    from mudiff_hip import ops
    mode = dict(none=ops.PRO_NONE, affine=ops.PRO_AFFINE, silu=ops.PRO_AFFINE_SILU, lrelu=ops.PRO_LRELU)[pro]
    gen = torch.Generator().manual_seed(B * 7 + H + Cin + Cout + mode)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) / math.sqrt(Cin * 9)
    bias = torch.randn(Cout, generator=gen)
    sc, sh = torch.rand(B, Cin, generator=gen) + 0.5, torch.randn(B, Cin, generator=gen)
    xv = ops.View.from_nchw(g(x))
    assert ops.TILE_NAMES[ops.conv_tile(xv, Cout)] == tile          # the label is the tile that runs (mud_conv2d_mfma_tile)
    assert ops.conv_prec_supported(xv, Cout, mode, ops.PREC_16X1)
    prol = None if mode == ops.PRO_NONE else (g(sc), g(sh), mode) if mode != ops.PRO_LRELU else (None, None, mode)
    y = ops.conv(xv, ops.pack_conv_weight(g(w), prec=ops.PREC_16X1), 3, Cout, mfma=True, pro=prol, bias=g(bias), prec=ops.PREC_16X1).to_nchw()
    # PRO_NONE: exact operands, a tight bar; with a prologue the fp32 value before the rounding may differ in its last bit (fast SiLU,
    # fma): a rare fp16 operand one ulp away, hence a looser multiple
    _check(y, _h16(_pro_host(x, sc, sh, mode)), _h16(w), bias=bias, mult=1.0 if mode == ops.PRO_NONE else 4.0, tag=f'{tile} pro={pro}')
    # and it is not the 16x3 result: the plan really ran
    y3 = ops.conv(xv, ops.pack_conv_weight(g(w)), 3, Cout, mfma=True, pro=prol, bias=g(bias)).to_nchw()
    assert float((y - y3).abs().max()) > 1e-5


def _fused_launch_splits(xv, Cout):
    """Would the fused-skip launch of this shape be split over K (mud_conv2d_mfma_splitk_bytes with skip_w and arrival counters set,
    as ops.conv sets them)?"""
    import ctypes as C
    import mudiff_hip
    from mudiff_hip import ops
    a = mudiff_hip.ConvArgs()
    a.x, a.B, a.H, a.W, a.Cin, a.ldx, a.ks, a.stride, a.pad = xv.ptr, xv.B, xv.H, xv.W, xv.C, xv.ld, 3, 1, 1
    a.out, a.Cout, a.ldo, a.pro_mode, a.skip_w = xv.ptr, Cout, Cout, ops.PRO_AFFINE_SILU, xv.ptr
    cnt = ops.splitk_counters(torch.device(DEV))
    a.splitk_counters, a.splitk_ncounters = C.c_void_p(cnt.data_ptr()), cnt.numel()
    return mudiff_hip.load().mud_conv2d_mfma_splitk_bytes(C.byref(a)) > 0


@pytest.mark.parametrize('B,H,W,Cin,Cout,tile', [(4, 128, 128, 64, 128, '8X2'), (2, 256, 256, 48, 64, '16X1'), (2, 20, 37, 48, 96, 'MT1'),
                                                 (1, 64, 64, 512, 256, 'MT1 split-K')])
def test_fused_skip_launch(B, H, W, Cin, Cout, tile):
    """The DUAL kernels: the 3x3 products take the plan, the 1x1 skip conv's own stay 16-bit x 3 - the same bits as under 16x3."""
    from mudiff_hip import ops
    gen = torch.Generator().manual_seed(Cin * 3 + Cout + B)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) / math.sqrt(Cin * 9)
    w2 = torch.randn(Cout, Cin, 1, 1, generator=gen) / math.sqrt(Cin)
    bias, bias_s = torch.randn(Cout, generator=gen), torch.randn(Cout, generator=gen)
    sc, sh = torch.rand(B, Cin, generator=gen) + 0.5, torch.randn(B, Cin, generator=gen)
    xv, w2p = ops.View.from_nchw(g(x)), ops.pack_conv_weight(g(w2))
    assert ops.TILE_NAMES[ops.conv_tile(xv, Cout, skip=True)] == tile.split()[0]
    assert ops.fused_skip_ok(xv, Cout, ops.PRO_AFFINE_SILU) and ops.conv_prec_supported(xv, Cout, ops.PRO_AFFINE_SILU, ops.PREC_16X1, skip=True)
    assert _fused_launch_splits(xv, Cout) == ('split-K' in tile)         # the split-K case really is one
    pro = (g(sc), g(sh), ops.PRO_AFFINE_SILU)
    out, skip = ops.View.empty(B, H, W, Cout, DEV), ops.View.empty(B, H, W, Cout, DEV)
    ops.conv(xv, ops.pack_conv_weight(g(w), prec=ops.PREC_16X1), 3, Cout, mfma=True, pro=pro, bias=g(bias), out=out, skip=(w2p, g(bias_s), skip),
             prec=ops.PREC_16X1)
    _check(out.to_nchw(), _h16(_pro_host(x, sc, sh, ops.PRO_AFFINE_SILU)), _h16(w), bias=bias, mult=4.0, tag=f'DUAL {tile} 3x3')
    ref_s = F.conv2d(x.double(), w2.double(), bias_s.double())
    es = float((skip.to_nchw().cpu().double() - ref_s).abs().max())
    print(f'DUAL {tile} 1x1 skip vs unrounded fp64: {es:.2e}')
    assert es <= 1e-4                                               # the 16x3 bar of test_conv_with_fused_skip_conv
    out3, skip3 = ops.View.empty(B, H, W, Cout, DEV), ops.View.empty(B, H, W, Cout, DEV)
    ops.conv(xv, ops.pack_conv_weight(g(w)), 3, Cout, mfma=True, pro=pro, bias=g(bias), out=out3, skip=(w2p, g(bias_s), skip3))
    assert torch.equal(skip.to_nchw(), skip3.to_nchw())
    assert int(ops.splitk_counters(torch.device(DEV)).abs().sum()) == 0


@pytest.mark.parametrize('B,H,W,Cin,Cout', [(1, 64, 64, 256, 256), (1, 32, 32, 384, 128)])
def test_split_k_small_grid(B, H, W, Cin, Cout):
    """Small grids split over K (slabs reduced by the last workgroup): every epilogue term on, against the definition."""
    from mudiff_hip import ops
    gen = torch.Generator().manual_seed(Cin + Cout)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) / math.sqrt(Cin * 9)
    bias, res = torch.randn(Cout, generator=gen), torch.randn(B, Cout, H, W, generator=gen)
    sc, sh = torch.rand(B, Cin, generator=gen) + 0.5, torch.randn(B, Cin, generator=gen)
    xv = ops.View.from_nchw(g(x))
    assert ops.conv3x3_would_split_k(xv, Cout)
    y = ops.conv(xv, ops.pack_conv_weight(g(w), prec=ops.PREC_16X1), 3, Cout, mfma=True, pro=(g(sc), g(sh), ops.PRO_AFFINE_SILU), bias=g(bias),
                 res=ops.View.from_nchw(g(res)), prec=ops.PREC_16X1).to_nchw()
    _check(y, _h16(_pro_host(x, sc, sh, ops.PRO_AFFINE_SILU)), _h16(w), bias=bias, res=res, mult=4.0, tag=f'split-K {H}x{W} {Cin}->{Cout}')
    assert int(ops.splitk_counters(torch.device(DEV)).abs().sum()) == 0


def test_saturation_gives_finite_saturated_results():
    """Inputs and weights beyond +-65504 are rounded to +-65504 (not inf): finite results equal to the saturated definition."""
    from mudiff_hip import ops
    gen = torch.Generator().manual_seed(9)
    B, H, W, Cin, Cout = 2, 16, 40, 32, 64
    x = torch.randn(B, Cin, H, W, generator=gen)
    x[:, :4] *= 1e6                                                 # far beyond fp16's range
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) / math.sqrt(Cin * 9)
    w[:2, :2] = 1e5
    w[2:4, :2] = -1e5
    y = ops.conv(ops.View.from_nchw(g(x)), ops.pack_conv_weight(g(w), prec=ops.PREC_16X1), 3, Cout, mfma=True, prec=ops.PREC_16X1).to_nchw()
    assert torch.isfinite(y).all()
    _check(y, _h16(x), _h16(w), tag='saturation')


def _forward_record(g1, g2, cfg, B, plan):
    from mudiff_hip import ops, precision
    H = cfg.image_size
    gen = torch.Generator().manual_seed(B)
    x, c1, c2, c3 = (g(torch.tanh(torch.randn(B, 1, H, H, generator=gen))) for _ in range(4))
    z, t = g(torch.randn(B, cfg.nz, generator=gen)), g(torch.randint(0, cfg.num_timesteps, (B,), generator=gen))
    with ops.prec_plan(plan), precision.launch_record() as rec:
        y1 = g1(x, c1, c2, c3, t, z)
        g2(x, c1, c2, c3, t, z, y1)
    torch.cuda.synchronize()
    return rec.launches


def _build(cfg, seed=1234):
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
    g1.load_state_dict(O.make_state_dict(cfg, 'g1', seed))
    g2.load_state_dict(O.make_state_dict(cfg, 'g2', seed))
    return g1.to(DEV).eval(), g2.to(DEV).eval()


def test_launch_record_covers_every_3x3_launch_of_g1_g2():
    """Config 3 shapes at B = 1 and B = 32: under 'fp16' every 3x3 matrix-core launch runs MUD_PREC_16X1 (sub2 pyramid convs, fused
    skip convs and split-K launches included) and nothing else changes plan; under 'auto' no launch runs it, and the launches are
    the same ones."""
    from mudiff_hip import ops
    cfg = O.default_config()
    g1, g2 = _build(cfg)
    for B in (1, 32):
        rec = _forward_record(g1, g2, cfg, B, 'fp16')
        conv3 = [r for r in rec if r.mfma and r.ks == 3]
        other = [r for r in rec if not (r.mfma and r.ks == 3)]
        print(f'B={B}: {len(conv3)} 3x3 matrix-core launches ({sum(r.sub2 for r in conv3)} sub2, {sum(r.skip for r in conv3)} with the skip '
              f'conv), {len(other)} others ({sum(r.ks == 1 for r in other)} 1x1, {sum(not r.mfma for r in other)} direct)')
        assert conv3 and other and any(r.sub2 for r in conv3) and any(r.skip for r in conv3)
        assert all(r.prec == ops.PREC_16X1 for r in conv3), [r for r in conv3 if r.prec != ops.PREC_16X1]
        assert all(r.prec == ops.PREC_16X3 for r in other)
        # every launch is named by its state_dict name ('feat_att' for G2's merged gate convs), the sub2 pyramid convs included
        keys = set(g1.state_dict()) | set(g2.state_dict())
        assert all(r.layer == 'feat_att' or r.layer + '.weight' in keys for r in conv3), [r.layer for r in conv3 if r.layer + '.weight' not in keys]
        sub2 = [r.layer for r in conv3 if r.sub2]
        assert len(set(sub2)) == len(sub2)
        auto = _forward_record(g1, g2, cfg, B, 'auto')
        same = lambda rs: [(r.layer, r.ks, r.mfma, r.shape, r.sub2, r.skip, r.pro) for r in rs]      # noqa: E731
        assert same(auto) == same(rec)
        # under 'auto' every launch runs what ops.choose_prec gives for it (the rule is unchanged; the sub2 convs, which before took
        # no plan at all, stay 16x3), every other launch 16x3
        with ops.prec_plan('auto'):
            for r in auto:
                if r.mfma and r.ks == 3:
                    Bx, Hx, Wx, Cx, Co = r.shape
                    v = ops.View(torch.empty(16, device=DEV), Bx, Hx, Wx, Cx)        # (only sizes are looked at)
                    want = ops.PREC_16X3 if r.sub2 else ops.choose_prec(v, Co, r.pro, skip=r.skip, sub2=r.sub2)
                else:
                    want = ops.PREC_16X3
                assert r.prec == want, (r, want)
        if B == 32:
            assert any(r.prec == ops.PREC_FP8X for r in auto)
    with pytest.raises(RuntimeError, match='nest'):
        from mudiff_hip import precision
        with precision.launch_record(), precision.launch_record():
            pass


def _emulate(cfg, conds, x_init, zs, noises, jitter=None):
    """The oracle sampler with fp16-rounded operands (activations after their prologue, weights) on exactly the 3x3 convs the library
    runs on the matrix cores (scripts/exp_operand_rounding.py's patch of F.conv2d) -> (per-step outputs, rounded convs per G1 + G2
    pass).  jitter: a torch.Generator - every such activation is first moved by one fp32 ulp up or down at random, i.e. what two
    implementations whose fp32 intermediates differ in the last bit feed the rounding."""
    from backbones.layerspp import ConvParam
    orig, rounded = F.conv2d, []

    def patched(x, w, *args, **kw):
        stride = kw.get('stride', args[1] if len(args) > 1 else 1)
        O_, I_, k = w.shape[0], w.shape[1], w.shape[-1]
        if k == 3 and (ConvParam.uses_mfma(O_, I_, 3) if stride in (1, (1, 1)) else (I_ % 4 == 0 and I_ >= 8)):
            rounded.append((I_, O_))
            if jitter is not None:
                x = x * (1 + (torch.randint(0, 2, x.shape, generator=jitter).float() * 2 - 1) * 2.0 ** -23)
            x, w = x.half().float(), w.half().float()
        return orig(x, w, *args, **kw)

    sd1, sd2 = O.make_state_dict(cfg, 'g1', 1234), O.make_state_dict(cfg, 'g2', 1234)
    O.F.conv2d = patched
    try:
        _, steps = O.sample_from_model(O.PosteriorCoefficients(cfg), sd1, sd2, cfg, *conds, x_init, zs, noises, return_steps=True)
    finally:
        O.F.conv2d = orig
    return steps, len(rounded) // cfg.num_timesteps


def _check_rounded_set(g1, g2, cfg, B, per_pass):
    """The oracle's rounded convs are the launches that took the plan (G2's merged gate launch counts as the convs it merges)."""
    from mudiff_hip import ops
    launches = [r for r in _forward_record(g1, g2, cfg, B, 'fp16') if r.prec == ops.PREC_16X1]
    gates = [r for r in launches if r.layer == 'feat_att']
    n_gate_convs = sum(1 for n, m in g2.named_modules() if n.startswith('feat_att') and isinstance(m, torch.nn.Conv2d))
    assert per_pass == len(launches) - len(gates) + n_gate_convs * len(gates), (per_pass, len(launches), len(gates), n_gate_convs)


def test_sampler_parity_against_the_emulated_reference():
    """Config 2 fixture (B = 1, 256x256, 4 steps) through the captured sampler under 'fp16', against the oracle run with fp16-rounded
    operands on exactly the 3x3 convs the library runs on the matrix cores, and against the reference's recorded outputs (<= 5e-2).
    The emulation cannot be met to 1e-3: moving every rounded activation of the EMULATION by one fp32 ulp moves its own outputs by
    ~1e-2 per step (operands on an fp16 rounding boundary flip, and the sampler amplifies the flips).  That distance, measured here,
    is the floor: the library must sit within 2x of it (and within 2.5e-2 in any case)."""
    from mudiff_hip import ops, sampling as S
    gd = load_golden('full_cfg2.npz')
    cfg = O.default_config()
    g1, g2 = _build(cfg)
    conds = demo_conds()
    x_init, zs, noises = sampler_inputs(cfg, 1)
    emu, per_pass = _emulate(cfg, conds, x_init, zs, noises)
    floor, _ = _emulate(cfg, conds, x_init, zs, noises, jitter=torch.Generator().manual_seed(1))
    _check_rounded_set(g1, g2, cfg, 1, per_pass)
    with ops.prec_plan('fp16'):
        sampler = S.GraphSampler(S.Posterior_Coefficients(cfg, DEV), g1, g2, cfg, 1, 256, 256, DEV)
    _, steps = sampler.sample(*[g(c) for c in conds], g(x_init), 4, zs=[g(z) for z in zs], noises=[g(n) for n in noises], return_steps=True)
    for k, (st, em, fl) in enumerate(zip(steps, emu, floor)):
        e_emu = max(float((v.cpu().double() - e.double()).abs().max()) for v, e in zip(st, em))
        e_floor = max(float((f.double() - e.double()).abs().max()) for f, e in zip(fl, em))
        e_ref = max(float((v.cpu().double() - gd[f'step{k}.{nm}'].double()).abs().max()) for v, nm in zip(st, ('x01', 'x02', 'xnew')))
        print(f'cfg2 fp16 plan step {k}: max-abs vs emulation {e_emu:.2e} (emulation vs its 1-ulp-jittered self {e_floor:.2e}), '
              f'vs reference {e_ref:.2e}')
        assert e_emu <= min(2.0 * e_floor, 2.5e-2) and e_ref <= 5e-2


def test_sampler_parity_wide_config3_batch32():
    """The wide config-3 fixture (16 BraTS-shaped slices over the four target orderings) as ONE batch of 32 (two replicas) through the
    captured sampler under 'fp16' - the 8-wave tiles and fused-skip tiles of the speed claims, end to end.  Every step against the
    emulated oracle (the 16 distinct slices, same draws) and x_new against the reference's own runs; same rounded-conv count check and
    bars as at B = 1 (the jittered-emulation floor is measured there; here the fixed bar of 2.5e-2 holds)."""
    from helpers import wide_cfg3_case
    from mudiff_hip import ops, sampling as S
    cfg = O.default_config()
    g1, g2 = _build(cfg)
    case = wide_cfg3_case(cfg, copies=2)
    half = lambda t: t[:16].contiguous()                            # noqa: E731  (one replica: the 16 distinct slices)
    emu, per_pass = _emulate(cfg, [half(c) for c in case['conds']], half(case['x_init']), [half(z) for z in case['zs']],
                             [half(n) for n in case['noises']])
    _check_rounded_set(g1, g2, cfg, 32, per_pass)
    with ops.prec_plan('fp16'):
        sampler = S.GraphSampler(S.Posterior_Coefficients(cfg, DEV), g1, g2, cfg, 32, 256, 256, DEV)
    _, steps = sampler.sample(*[g(c) for c in case['conds']], g(case['x_init']), 4, zs=[g(z) for z in case['zs']],
                              noises=[g(n) for n in case['noises']], return_steps=True)
    for k, (st, em) in enumerate(zip(steps, emu)):
        e_emu = max(float((v.cpu().double().view(2, 16, -1) - e.double().view(1, 16, -1)).abs().max()) for v, e in zip(st, em))
        e_ref = float((st[2].cpu().double().view(2, 16, -1) - case['refs'][k].double().view(1, 16, -1)).abs().max())
        print(f'cfg3 wide B=32 fp16 plan step {k}: max-abs vs emulation {e_emu:.2e}, x_new vs reference {e_ref:.2e}')
        assert e_emu <= 2.5e-2 and e_ref <= 5e-2


def test_graph_equals_eager_bitwise_under_deterministic():
    code = r'''
import sys, torch
sys.path.insert(0, "tests")
from helpers import SMALL_CFGS, sampler_inputs, small_conds
from oracle import mudiff_oracle as O
from mudiff_hip import ops, precision, sampling as S
from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
assert ops.DETERMINISTIC
cfg = O.default_config(**SMALL_CFGS["s32"])
g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
g1.load_state_dict(O.make_state_dict(cfg, "g1", 1234)); g2.load_state_dict(O.make_state_dict(cfg, "g2", 1234))
g1, g2 = g1.cuda().eval(), g2.cuda().eval()
conds = [c.cuda() for c in small_conds(cfg)]
x_init, zs, noises = sampler_inputs(cfg, 2)
coef = S.Posterior_Coefficients(cfg, "cuda:0")
with ops.prec_plan("fp16"):
    with precision.launch_record() as rec:
        eager = S.sample_from_model(coef, g1, conds[0], g2, conds[1], conds[2], cfg.num_timesteps, x_init.cuda(), None, cfg,
                                    zs=[z.cuda() for z in zs], noises=[n.cuda() for n in noises])
    assert any(r.prec == ops.PREC_16X1 for r in rec.launches)
    sampler = S.GraphSampler(coef, g1, g2, cfg, 2, 32, 32, "cuda:0")
graphed = sampler.sample(conds[0], conds[1], conds[2], x_init.cuda(), cfg.num_timesteps, zs=[z.cuda() for z in zs], noises=[n.cuda() for n in noises])
assert torch.equal(eager, graphed), float((eager - graphed).abs().max())
off = S.sample_from_model(coef, g1, conds[0], g2, conds[1], conds[2], cfg.num_timesteps, x_init.cuda(), None, cfg,
                          zs=[z.cuda() for z in zs], noises=[n.cuda() for n in noises])
assert not torch.equal(off, eager)
print("GRAPH-EQ-EAGER-OK")
'''
    env = dict(os.environ, MUD_DETERMINISTIC='1', PYTHONPATH=os.pathsep.join([REPO, PKG, os.environ.get('PYTHONPATH', '')]))
    p = subprocess.run([sys.executable, '-c', code], cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0 and 'GRAPH-EQ-EAGER-OK' in p.stdout, p.stderr[-3000:]


def test_driver_cli_with_the_fp16_plan(tmp_path):
    from test_driver import _write_volumes
    data, out = tmp_path / 'data', tmp_path / 'out'
    _write_volumes(str(data), n=5, hw=32, seed=7)
    cfg = O.default_config(**SMALL_CFGS['s32'])
    os.makedirs(out / 'exp9')
    for which, name in (('g1', 'gen_diffusive_1'), ('g2', 'gen_diffusive_2')):
        torch.save(O.make_state_dict(cfg, which, 1234), out / 'exp9' / f'{name}.pth')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.environ.get('PYTHONPATH', '')]))
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MUD_PREC_PLAN'):
        env.pop(k, None)
    cmd = [sys.executable, '-m', 'mudiff_hip.driver', '--input_path', str(data), '--output_path', str(out), '--exp', 'exp9', '--target_modality', 'T2',
           '--image_size', '32', '--num_channels_dae', '32', '--ch_mult', '1', '2', '4', '--attn_resolutions', '16', '--batch_size', '4',
           '--prec_plan', 'fp16', '--device_metrics']
    p = subprocess.run(cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [ln for ln in p.stderr.splitlines() if 'Average PSNR' in ln]
    assert line and re.search(r'over 5 slices .*prec_plan: fp16$', line[0]), line
    pngs = sorted(os.listdir(out / 'generated_samples' / 'pred'))
    assert pngs == [f'pred_{i:05d}.png' for i in range(5)]
    assert np.isfinite(float(re.search(r'Average PSNR: (\S+) dB', line[0]).group(1)))
