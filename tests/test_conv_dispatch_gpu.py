"""GPU: mud_conv2d_mfma's table of built kernels (csrc/conv_mfma.hip, kCmRows), key by key: (tile, prologue, fused skip conv, plan).

BUILT below is written by hand from the list the table was specified with - it is NOT read from the library: 5 tiles x 4 prologues under
the two fp16 plans, the fp8 cross-term plan on the three 8-wave tiles without prologue and with AdaGN + SiLU, and the fused skip conv
(AdaGN + SiLU only) on 8X2, 16X1 and MT1 under the fp16 plans, on 8X2 and 16X1 under the fp8 plan.  Every built key is asked for through
the queries (ops.conv_tile, ops.conv_prec_supported), launched with a plain epilogue (+ bias) on the ragged shapes of
test_conv_forms_gpu (SHAPES: channel slices of NaN- / sentinel-filled buffers) and compared with fp64 under that file's bar for the plan:
  16x3  max-abs <= 3e-5 x max(1, max|ref|)
  16x1  helpers.check_fp16_definition (1 x K 2^-24 sum|a w| without a prologue, 4 x with one)
  fp8x  rms error <= 4e-5 of the convolution's rms + 1e-6 (test_conv_fp8x_plan_vs_fp64)
  fused skip conv: the 1x1 skip output at 1e-4 under every plan (its products stay 16-bit x 3), the 3x3 output at 1e-4 under the default
  plan and at the plan's own bar above under the other two (test_fp16_plan_gpu.test_fused_skip_launch)
Every key that is NOT built must be refused the same way by both sides: the query says no, mud_conv2d_mfma returns an error that names
the plan or the form, and the sentinel-filled output is untouched.  The in_up2 / in_s2d rows are launched per tile and plan by
test_in_up2.py (TILES x _plans) and test_pyr_s2d.py (TILES x both fp16 plans)."""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import check_fp16_definition, h16, pro_host
from test_conv_forms_gpu import DEV, SENTINEL, SHAPES, _problem, _result, _slice_in, _slice_out, g

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TILES = ['8X1R', '8X2', '16X1', 'MT2', 'MT1']                    # SHAPES' names: each is the tile a plain launch of that shape takes
PROS = ['none', 'affine', 'lrelu', 'silu']
PLANS = ['16x3', '16x1', 'fp8x']
SKIP_TILE = {'8X1R': 'MT1', '8X2': '8X2', '16X1': '16X1', 'MT2': 'MT1', 'MT1': 'MT1'}      # the fused skip conv's tile on the same shape

# (tile, prologue, fused skip conv, plan)
BUILT = ({(t, p, False, plan) for t in TILES for p in PROS for plan in ('16x3', '16x1')}
         | {(t, 'silu', True, plan) for t in ('8X2', '16X1', 'MT1') for plan in ('16x3', '16x1')}
         | {(t, p, False, 'fp8x') for t in ('8X2', '16X1', '8X1R') for p in ('none', 'silu')}
         | {(t, 'silu', True, 'fp8x') for t in ('8X2', '16X1')})
assert len(BUILT) == 40 + 6 + 6 + 2

# one shape after the other (the Problem cache holds one): every plain key, then the fused skip conv with every prologue on the shape's
# fused tile.  MT1's own shape has too few pixels to matter twice: the fused MT1 rows run on the 8X1R and MT2 shapes, whose fused
# launch falls to MT1 at a chip-filling grid (the 'tile falls to MT1' case of the fp8 plan)
CASES = [(name, pro, skip, plan) for name in TILES for skip in (False, True) for plan in PLANS for pro in PROS if not (skip and name == 'MT1')]
IDS = [f'{n}-{pl}-{pr}{"-skip" if s else ""}' for n, pr, s, pl in CASES]


def _codes():
    from mudiff_hip import ops
    return (dict(zip(PROS, (ops.PRO_NONE, ops.PRO_AFFINE, ops.PRO_LRELU, ops.PRO_AFFINE_SILU))),
            dict(zip(PLANS, (ops.PREC_16X3, ops.PREC_16X1, ops.PREC_FP8X))))


def _operand(p, pro):
    """The prologued input in fp32 as the kernels form it before rounding to fp16.  'affine' is one fused multiply-add there
    (cm_stage4: fmaf) - x * sc exact in fp64, one rounding of the sum - where pro_host's product rounds first; the SiLU form was moved
    off the fp16 midpoints by Problem._off_midpoints and is pro_host's."""
    from mudiff_hip import ops
    if pro == 'affine':
        return (p.x.double() * p.sc.double()[:, :, None, None] + p.sh.double()[:, :, None, None]).float()
    return pro_host(p.x, p.sc, p.sh, _codes()[0][pro])


def _check_plan(p, pro, plan, y, tag):
    """The 3x3 output `y` (NCHW, host) of a plain-epilogue (+ bias) launch against fp64 under the plan's bar."""
    ref = p.conv(pro, torch.float64) + p.bias.double()[None, :, None, None]
    e32 = float(((p.conv(pro, torch.float32) + p.bias[None, :, None, None]).double() - ref).abs().max())
    if plan == '16x3':
        err, bar = float((y.double() - ref).abs().max()), 3e-5 * max(1.0, float(ref.abs().max()))
        print(f'{tag}: max-abs vs fp64 {err:.2e} (bar {bar:.2e}), torch fp32 {e32:.2e}')
        assert err <= bar
    elif plan == '16x1':
        check_fp16_definition(y, h16(_operand(p, pro)), h16(p.w), bias=p.bias, mult=1.0 if pro == 'none' else 4.0, tag=tag)
    else:
        rms = lambda e: float(e.pow(2).mean().sqrt())      # noqa: E731
        e8, bar = rms(y.double() - ref), 4e-5 * rms(p.conv(pro, torch.float64)) + 1e-6
        print(f'{tag}: rms err {e8:.2e} (bar {bar:.2e}), torch fp32 max-abs {e32:.2e}')
        assert e8 <= bar


def _untouched(view):
    return bool((view.base == SENTINEL).all())


@pytest.mark.parametrize('name,pro,skip,plan', CASES, ids=IDS)
def test_every_key_is_launched_or_refused_by_query_and_dispatcher_alike(name, pro, skip, plan):
    import mudiff_hip
    from mudiff_hip import ops
    pro_code, prec_code = _codes()
    mode, prec = pro_code[pro], prec_code[plan]
    p = _problem(name, True)
    tile = SKIP_TILE[name] if skip else p.tile
    xv = _slice_in(p.x)
    assert ops.TILE_NAMES[ops.conv_tile(xv, p.Cout, skip=skip, pro_mode=mode, prec=prec)] == tile
    built = (tile, pro, skip, plan) in BUILT
    tag = f'{tile} {p.B}x{p.H}x{p.W} {p.Cin}->{p.Cout} pro {pro}{" + skip conv" if skip else ""} {plan}'
    we = ops.fp8x_weight_exponent(p.w) if plan == 'fp8x' else 0
    kw = dict(mfma=True, prec=prec, w_exp=we, bias=g(p.bias), pro=None if pro == 'none' else (None, None, mode) if pro == 'lrelu' else (g(p.sc), g(p.sh), mode))
    out = _slice_out(p.B, p.H, p.W, p.Cout)
    if skip:
        gen = torch.Generator().manual_seed(p.Cin + p.Cout)
        w2, bias_s = torch.randn(p.Cout, p.Cin, 1, 1, generator=gen) / math.sqrt(p.Cin), torch.randn(p.Cout, generator=gen)
        skip_out = _slice_out(p.B, p.H, p.W, p.Cout)
        kw.update(skip=(ops.pack_conv_weight(g(w2)), g(bias_s), skip_out))
    wp = ops.pack_conv_weight(g(p.w), prec=prec, w_exp=we)
    # the default plan's query speaks of the plan alone (every launch has it): a fused skip conv without AdaGN + SiLU is refused by form
    if plan != '16x3':
        assert ops.conv_prec_supported(xv, p.Cout, mode, prec, skip=skip) == built, tag
    else:
        assert ops.conv_prec_supported(xv, p.Cout, mode, prec, skip=skip)
    if built:
        ops.conv(xv, wp, 3, p.Cout, out=out, **kw)
        if not skip:
            return _check_plan(p, pro, plan, _result(out), tag)
        y, ys = _result(out), _result(skip_out)
        ref_s = F.conv2d(p.x.double(), w2.double(), bias_s.double())
        e2 = float((ys.double() - ref_s).abs().max())
        print(f'{tag}: 1x1 skip output {e2:.2e} (bar 1e-4)')
        assert e2 <= 1e-4
        if plan == '16x3':
            e1 = float((y.double() - (p.conv(pro, torch.float64) + p.bias.double()[None, :, None, None])).abs().max())
            print(f'{tag}: 3x3 output {e1:.2e} (bar 1e-4)')
            assert e1 <= 1e-4
        else:
            _check_plan(p, pro, plan, y, tag)
        return
    # fused skip conv with another prologue: the form is refused whatever the plan; else the plan has no kernel for (tile, prologue)
    words = 'fused skip conv' if skip and pro != 'silu' else 'MUD_PREC_FP8X is not built'
    with pytest.raises(mudiff_hip.MudiffHipError, match=words):
        ops.conv(xv, wp, 3, p.Cout, out=out, **kw)
    torch.cuda.synchronize()
    assert _untouched(out) and (not skip or _untouched(skip_out)), f'{tag}: refused, yet something was written'


def test_the_cases_reach_every_built_key_and_every_kind_of_refusal():
    """(no launch) CASES against the hand-written list: every built key is launched, and the keys that are not built hold each kind the
    dispatcher must refuse."""
    keys = {((SKIP_TILE[n] if s else n), pr, s, pl) for n, pr, s, pl in CASES}
    assert BUILT <= keys
    missing = keys - BUILT
    assert {(t, pr) for t, pr, s, pl in missing if pl == 'fp8x' and not s} == \
        {(t, pr) for t in ('MT2', 'MT1') for pr in PROS} | {(t, pr) for t in ('8X2', '16X1', '8X1R') for pr in ('affine', 'lrelu')}
    assert {(t, pr, pl) for t, pr, s, pl in missing if s and pr != 'silu'} == {(t, pr, pl) for t in ('8X2', '16X1', 'MT1') for pr in PROS[:3] for pl in PLANS}
    assert ('MT1', 'silu', True, 'fp8x') in missing
    assert not [k for k in missing if k[3] != 'fp8x' and not k[2]]      # the fp16 plans have every plain key


@pytest.mark.parametrize('plan', ['16x1', 'fp8x'])
@pytest.mark.parametrize('pro', PROS)
def test_the_1x1_kernel_has_the_default_plan_only(pro, plan):
    """ks = 1 under MUD_PREC_16X1 / MUD_PREC_FP8X: the query says no (16x3: yes), the launch is refused by name, nothing is written.
    (Neither plan has a packed 1x1 operand: the weights are the default plan's, which a refused launch never reads.)"""
    import mudiff_hip
    from mudiff_hip import ops
    pro_code, prec_code = _codes()
    mode, prec = pro_code[pro], prec_code[plan]
    B, H, W, Cin, Cout = 3, 5, 7, 36, 40
    gen = torch.Generator().manual_seed(Cin + Cout)
    x, w = torch.randn(B, Cin, H, W, generator=gen), torch.randn(Cout, Cin, 1, 1, generator=gen) / math.sqrt(Cin)
    sc, sh = torch.rand(B, Cin, generator=gen) + 0.5, torch.randn(B, Cin, generator=gen)
    xv = _slice_in(x)
    lib = mudiff_hip.load()
    ask = lambda pr: lib.mud_conv2d_mfma_prec_supported(ops._query_args(B, H, W, Cin, xv.ld, Cout, xv.ptr, pro_mode=mode, ks=1, pad=0), pr)   # noqa: E731
    assert ask(ops.PREC_16X3) == 1 and ask(prec) == 0
    out = _slice_out(B, H, W, Cout)
    kw = dict(mfma=True, out=out, pro=None if pro == 'none' else (None, None, mode) if pro == 'lrelu' else (g(sc), g(sh), mode))
    with pytest.raises(mudiff_hip.MudiffHipError, match='MUD_PREC_16X1' if plan == '16x1' else 'MUD_PREC_FP8X is not built'):
        ops.conv(xv, ops.pack_conv_weight(g(w)), 1, Cout, prec=prec, **kw)
    torch.cuda.synchronize()
    assert _untouched(out)
    ops.conv(xv, ops.pack_conv_weight(g(w)), 1, Cout, **kw)             # the default plan runs: every prologue of the 1x1 kernel
    ref = F.conv2d(pro_host(x, sc, sh, mode).double(), w.double())
    err, bar = float((_result(out).double() - ref).abs().max()), 3e-5 * max(1.0, float(ref.abs().max()))
    print(f'1x1 {B}x{H}x{W} {Cin}->{Cout} pro {pro}: max-abs vs fp64 {err:.2e} (bar {bar:.2e})')
    assert err <= bar
