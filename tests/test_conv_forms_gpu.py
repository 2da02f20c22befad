"""GPU: the matrix-core convolution (csrc/conv_mfma.hip) on every workgroup tile at ragged sizes, with every epilogue term, against
torch in fp64 built from the same fp32 inputs.

The tile follows from the workgroup count (mud_conv2d_mfma_tile), so a large batch of tiny images reaches every tile for a few MB:
11 x 35 or 19 x 35 images (ragged last row group, ragged second column tile, odd so that sub2 applies), input channels with a ragged
last 16-channel chunk, output channels that are no multiple of 32 - and, for the scalar epilogue, no multiple of 4.  Every case first
asserts the tile it is named for through the query.  Operands are channel slices (offset 8, ld = C + 16) of wider buffers whose other
channels hold NaN on the input side and a sentinel on the output side: a read outside a slice shows up as NaN, a write as a lost
sentinel.  Bars are the project's: max-abs <= 3e-5 x max(1, max|ref|) for the default fp16 x 3 plan (test_conv_mfma_split_precision,
same input scaling), the definition bound of helpers.check_fp16_definition for MUD_PREC_16X1, the rms bar of
test_conv_fp8x_plan_vs_fp64 for MUD_PREC_FP8X, 1e-4 for both outputs of the fused skip conv (test_conv_with_fused_skip_conv) and 2e-6
of the largest sum for the statistics (test_conv_split_k_small_grids).  Every case prints its tile and its error, with torch's own fp32
error against fp64 on the same inputs beside it."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import check_fp16_definition, h16, pro_host

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = 'cuda:0'
SENTINEL = -12345.0
PAD, OFF = 16, 8                    # a slice sits at channel offset 8 of a buffer 16 channels wider
INV_SQRT2 = 1.0 / math.sqrt(2.0)

# name -> (tile, B, H, W, Cin, Cout that is a multiple of 4 but not of 32, Cout that is no multiple of 4)
SHAPES = {
    '8X1R': ('8X1R', 128, 11, 35, 20, 60, 62),
    '8X2': ('8X2', 64, 11, 35, 24, 100, 102),
    '16X1': ('16X1', 64, 19, 35, 68, 60, 62),
    'MT2': ('MT2', 128, 11, 35, 68, 60, 62),
    'MT1': ('MT1', 2, 11, 35, 20, 60, 62),
    'MT1-H5': ('MT1', 128, 5, 35, 20, 60, 62),           # H < 8 at a chip-filling batch
}
PROBLEMS = [(name, aligned) for name in SHAPES for aligned in (True, False)]
FORMS = ['a', 'a-contiguous', 'b', 'c', 'd', 'e', 'e-all', 'f', 'g']
# (shape, aligned Cout, plan, form), one shape after the other so that its fp64 convolutions are computed once: every form under the
# default plan, a / b / g under the single-pass plan, a / b under the fp8 cross-term plan on the three tiles it is built for
CASES = [(name, aligned, plan, form) for name, aligned in PROBLEMS
         for plan, forms in (('16x3', FORMS), ('16x1', ['a', 'b', 'g']), ('fp8x', ['a', 'b'] if SHAPES[name][0] in ('8X2', '16X1', '8X1R') else []))
         for form in forms]


def g(t):
    return t.to(DEV)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _slice_in(t_nchw):
    """-> View of the tensor as a channel slice of a wider NaN-filled device buffer."""
    from mudiff_hip import ops
    B, Cc, H, W = t_nchw.shape
    base = torch.full((B, H, W, Cc + PAD), float('nan'))
    base[..., OFF:OFF + Cc] = _nhwc(t_nchw)
    return ops.View(g(base), B, H, W, Cc + PAD).slice(OFF, Cc)


def _slice_out(B, H, W, Cc, arena=None):
    """-> View: a channel slice of a wider sentinel-filled device buffer (with per-channel statistics of the whole buffer)."""
    from mudiff_hip import ops
    wide = ops.View(torch.full((B, H, W, Cc + PAD), SENTINEL, device=DEV), B, H, W, Cc + PAD)
    if arena is not None:
        wide.stats = arena.take(B, Cc + PAD)
    return wide.slice(OFF, Cc)


def _result(out):
    """The launch's output (NCHW, on the host) after checking that nothing outside the slice was written, that every element of the
    slice was, and that the result is finite."""
    full = out.base.reshape(out.B, out.H, out.W, out.ld).cpu()
    inside = full[..., out.c0:out.c0 + out.C]
    assert bool((full[..., :out.c0] == SENTINEL).all()) and bool((full[..., out.c0 + out.C:] == SENTINEL).all()), 'wrote outside its slice'
    assert bool(torch.isfinite(inside).all()), 'non-finite output (NaN: a read outside an input slice)'
    assert not bool((inside == SENTINEL).any()), 'an output element was never written'
    return inside.permute(0, 3, 1, 2).contiguous()


def _check_stats(out, ref, tag):
    """(sum, sumsq) of the stored outputs, the bars of test_conv_split_k_small_grids; nothing accumulated outside the slice."""
    st = out.stats.cpu()
    s_ref, q_ref = ref.sum(dim=(2, 3)), (ref * ref).sum(dim=(2, 3))
    es = float((st[:, out.c0:out.c0 + out.C, 0] - s_ref).abs().max())
    eq = float((st[:, out.c0:out.c0 + out.C, 1] - q_ref).abs().max())
    bs, bq = 2e-6 * float(ref.abs().sum(dim=(2, 3)).max()), 2e-6 * float(q_ref.max())
    print(f'{tag}: statistics sum {es:.2e} (bar {bs:.2e}), sumsq {eq:.2e} (bar {bq:.2e})')
    assert es <= bs and eq <= bq
    assert float(st[:, :out.c0].abs().max()) == 0.0 and float(st[:, out.c0 + out.C:].abs().max()) == 0.0, 'statistics outside the slice'


class Problem:
    """The fp32 inputs of one (shape, Cout) and, made on first use and shared between forms and plans, the convolution of each
    prologue of them in fp64 and in torch's fp32."""

    def __init__(self, name, aligned=True, ks=3, dims=None, tile=None):
        self.name, self.ks = name, ks
        if dims is None:
            self.tile, B, H, W, Cin, c4, c2 = SHAPES[name]
            Cout = c4 if aligned else c2
        else:
            self.tile, (B, H, W, Cin, Cout) = tile, dims
        self.B, self.H, self.W, self.Cin, self.Cout = B, H, W, Cin, Cout
        gen = torch.Generator().manual_seed(1000 * B + 100 * H + 10 * Cin + Cout + ks)
        rn = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
        self.x = rn(B, Cin, H, W)                                           # unit variance
        self.w = rn(Cout, Cin, ks, ks) / math.sqrt(ks * ks * Cin)
        self.bias, self.bias2 = rn(Cout), rn(B, Cout)
        self.sc, self.sh = torch.rand(B, Cin, generator=gen) + 0.5, rn(B, Cin)
        self.res, self.other, self.emul = rn(B, Cout, H, W), rn(B, Cout, H, W), rn(B, Cout, H, W)
        self.gate = torch.rand(B, Cout, H, W, generator=gen)
        self.res_half = rn(B, Cout, H // 2, W // 2)
        self.emul_cout = (Cout // 2) & ~3 if Cout % 4 == 0 else (Cout // 2) | 1        # a multiple of 4 below Cout / an odd count
        self._conv = {}
        self._off_midpoints()

    def _off_midpoints(self):
        """Move the few inputs whose prologued value silu(sc * x + sh) lies within 2^-8 fp16 ulp (32 fp32 ulps) of an fp16 rounding
        midpoint.  The kernel's fp32 value there (fma, fast SiLU: a few fp32 ulps from torch's) may round the other way, and the
        definition bound of MUD_PREC_16X1 speaks of operands that are the same on both sides.  Measured without this at Cin = 20
        (K = 180, where one fp16 ulp on one operand is no longer small against 4 K 2^-24 sum|a w|): form b missed the bound by up to
        8.2 / 4 on 27 of 2 956 800 outputs, and every one of them was exactly +-1.000 fp16 ulp on a single operand that sat 0 to 2 fp32
        ulps from a midpoint, the rest of the error ~1e-6.  The inputs stay unit-variance fp32; every form and plan uses the moved x."""
        from mudiff_hip import ops
        for it in range(16):
            v = pro_host(self.x, self.sc, self.sh, ops.PRO_AFFINE_SILU).double()
            ulp = torch.clamp(2.0 ** (torch.floor(torch.log2(v.abs().clamp_min(1e-30))) - 10), min=2.0 ** -24)
            near = (((v - h16(v)).abs() / ulp) - 0.5).abs() < 2.0 ** -8
            if not bool(near.any()):
                return
            self.x[near] += 0.0071 * (1 + 0.173 * it)        # (no power of two: a step of whole fp16 ulps lands on the next midpoint)
        raise AssertionError('could not move the inputs off the fp16 midpoints')

    def pro(self, t, mode):
        """The prologue `mode` ('none' | 'affine' | 'silu' | 'lrelu') in t's precision."""
        if mode == 'none':
            return t
        if mode == 'lrelu':
            return F.leaky_relu(t, 0.2)
        a = t * self.sc.to(t.dtype)[:, :, None, None] + self.sh.to(t.dtype)[:, :, None, None]
        return F.silu(a) if mode == 'silu' else a

    def conv(self, mode, dtype, stride=1):
        """conv(prologue(x), w) without bias in `dtype` (stride 2: pad 0, the sub2 form's definition), computed once."""
        key = (mode, dtype, stride)
        if key not in self._conv:
            self._conv[key] = F.conv2d(self.pro(self.x.to(dtype), mode), self.w.to(dtype), stride=stride, padding=self.ks // 2 if stride == 1 else 0)
        return self._conv[key]

    def reference(self, form, dtype):
        """The form's definition in `dtype` (fp64: the reference; fp32: torch's own error on the same inputs)."""
        t = lambda v: v.to(dtype)                           # noqa: E731
        b1, b2 = t(self.bias)[None, :, None, None], t(self.bias2)[:, :, None, None]
        if form in ('a', 'a-contiguous'):
            return self.conv('none', dtype) + b1
        if form == 'b':                                     # the residual block's second conv
            return (self.conv('silu', dtype) + b1 + b2 + t(self.res)) * INV_SQRT2
        if form == 'b-affine':                              # (the 1x1 kernel: GroupNorm without SiLU in front of a NIN)
            return (self.conv('affine', dtype) + b1 + b2 + t(self.res)) * INV_SQRT2
        if form == 'c':
            return self.conv('affine', dtype) + b1
        if form == 'd':                                     # the critic's down block
            return F.leaky_relu(self.conv('lrelu', dtype) + b2, 0.2)
        if form in ('e', 'e-all'):                          # G2's gate conv: sigmoid, then emul on the first emul_cout channels / on all
            v = torch.sigmoid(self.conv('none', dtype) + b1)
            n = self.emul_cout if form == 'e' else self.Cout
            return torch.cat([v[:, :n] * t(self.emul)[:, :n], v[:, n:]], 1)
        if form == 'f':                                     # G2's fusion conv
            return t(self.gate) * (self.conv('none', dtype) + b1) + (1 - t(self.gate)) * t(self.other)
        if form == 'g':                                     # the input pyramid's stride-2 conv on the stride-1 kernel
            return (self.conv('none', dtype, stride=2) + b1 + t(self.res_half)) * INV_SQRT2
        raise KeyError(form)

    def launch(self, form, prec, arena, w_exp=0, split_k=True):
        """One launch of the form under plan `prec` on sliced (form 'a-contiguous': contiguous) views -> the output View."""
        from mudiff_hip import ops
        B, H, W, Cout = self.B, self.H, self.W, self.Cout
        plain = form == 'a-contiguous'
        xv = ops.View.from_nchw(g(self.x)) if plain else _slice_in(self.x)
        if self.ks == 3:
            assert ops.TILE_NAMES[ops.conv_tile(xv, Cout)] == self.tile, f'{self.name}: not the tile the case is named for'
        wp = ops.pack_conv_weight(g(self.w), prec=prec, w_exp=w_exp)
        kw = dict(mfma=True, prec=prec, w_exp=w_exp, split_k=split_k)
        aff = (g(self.sc), g(self.sh))
        if form in ('a', 'a-contiguous'):
            kw.update(bias=g(self.bias))
        elif form in ('b', 'b-affine'):
            kw.update(pro=(*aff, ops.PRO_AFFINE_SILU if form == 'b' else ops.PRO_AFFINE), bias=g(self.bias), bias2=g(self.bias2),
                      res=_slice_in(self.res), out_scale=INV_SQRT2)
        elif form == 'c':
            kw.update(pro=(*aff, ops.PRO_AFFINE), bias=g(self.bias))
        elif form == 'd':
            kw.update(pro=(None, None, ops.PRO_LRELU), bias2=g(self.bias2), act=ops.ACT_LRELU)
        elif form == 'e':
            kw.update(bias=g(self.bias), act=ops.ACT_SIGMOID, emul=_slice_in(self.emul[:, :self.emul_cout]), emul_cout=self.emul_cout)
        elif form == 'e-all':
            kw.update(bias=g(self.bias), act=ops.ACT_SIGMOID, emul=_slice_in(self.emul), emul_cout=0)
        elif form == 'f':
            kw.update(bias=g(self.bias), gate=(_slice_in(self.gate), _slice_in(self.other)))
        elif form == 'g':
            kw.update(bias=g(self.bias), res=_slice_in(self.res_half), out_scale=INV_SQRT2, sub2=True)
        Ho, Wo = (H // 2, W // 2) if form == 'g' else (H, W)
        if plain:
            out = ops.View(torch.full((B, Ho, Wo, Cout), SENTINEL, device=DEV), B, Ho, Wo, Cout)
        else:
            out = _slice_out(B, Ho, Wo, Cout, arena if form in ('b', 'b-affine', 'g') else None)
        ops.conv(xv, wp, self.ks, Cout, out=out, **kw)
        return out


@functools.lru_cache(maxsize=1)
def _problem(name, aligned):
    return Problem(name, aligned)


def _judge(p, form, y, tag):
    """The default plan's bar, with torch's fp32 error beside the launch's -> (launch error, torch fp32 error, bar)."""
    ref = p.reference(form, torch.float64)
    err = float((y.double() - ref).abs().max())
    e32 = float((p.reference(form, torch.float32).double() - ref).abs().max())
    bar = 3e-5 * max(1.0, float(ref.abs().max()))
    print(f'{tag}: max-abs vs fp64 {err:.2e} (bar {bar:.2e}), torch fp32 {e32:.2e}')
    assert err <= bar
    return ref


@pytest.mark.parametrize('name,aligned,plan,form', CASES, ids=[f'{n}-{"vec" if al else "scalar"}-{pl}-{f}' for n, al, pl, f in CASES])
def test_every_tile_form_and_plan(name, aligned, plan, form):
    """Every tile x (vector | scalar epilogue) x form x plan (see CASES) against fp64."""
    {'16x3': _default_plan, '16x1': _single_pass_plan, 'fp8x': _fp8x_plan}[plan](_problem(name, aligned), form)


def _default_plan(p, form):
    """fp16 x 3 (MUD_PREC_16X3): max-abs <= 3e-5 x max(1, max|ref|)."""
    from mudiff_hip import ops
    arena = ops.StatsArena(torch.device(DEV))
    out = p.launch(form, ops.PREC_16X3, arena)
    ref = _judge(p, form, _result(out), f'{p.tile} {p.B}x{p.H}x{p.W} {p.Cin}->{p.Cout} form {form} 16x3')
    if out.stats is not None:
        _check_stats(out, ref, f'{p.tile} form {form}')


def _single_pass_plan(p, form):
    """MUD_PREC_16X1 against its definition (fp16-rounded operands, exact products, fp32 accumulation): helpers.check_fp16_definition's
    bound, 1 x K 2^-24 sum|a w| without a prologue, 4 x with one (test_fp16_plan_gpu)."""
    from mudiff_hip import ops
    assert ops.conv_prec_supported(ops.View.from_nchw(g(p.x)), p.Cout, ops.PRO_AFFINE_SILU if form == 'b' else ops.PRO_NONE, ops.PREC_16X1, sub2=form == 'g')
    arena = ops.StatsArena(torch.device(DEV))
    out = p.launch(form, ops.PREC_16X1, arena)
    y = _result(out)
    tag = f'{p.tile} {p.B}x{p.H}x{p.W} {p.Cin}->{p.Cout} form {form} 16x1'
    if form == 'a':
        ref = check_fp16_definition(y, h16(p.x), h16(p.w), bias=p.bias, tag=tag)
    elif form == 'b':
        ref = check_fp16_definition(y, h16(pro_host(p.x, p.sc, p.sh, ops.PRO_AFFINE_SILU)), h16(p.w), bias=p.bias, bias2=p.bias2, res=p.res,
                                    scale=INV_SQRT2, mult=4.0, tag=tag)
    else:
        ref = check_fp16_definition(y, h16(p.x), h16(p.w), bias=p.bias, res=p.res_half, scale=INV_SQRT2, pick=lambda t: t[:, :, 1::2, 1::2], tag=tag)
    if out.stats is not None:
        _check_stats(out, y.double(), f'{p.tile} form {form} 16x1 (of the stored outputs)')
    e64 = float((y.double() - p.reference(form, torch.float64)).abs().max())
    e32 = float((p.reference(form, torch.float32).double() - p.reference(form, torch.float64)).abs().max())
    print(f'{tag}: max-abs vs unrounded fp64 {e64:.2e} (the plan is ~2^-11 per product: no bar), torch fp32 {e32:.2e}')
    # (the definition is the same convolution: operands rounded by 2^-11 each move an output by <= 2^-10 sum|a w|, and sum|a w| < 100 here)
    assert float((ref - p.reference(form, torch.float64)).abs().max()) < 0.1


def _fp8x_plan(p, form):
    """MUD_PREC_FP8X on its three tiles, weights packed with fp8x_weight_exponent: rms error <= 4e-5 of the convolution's rms
    (test_conv_fp8x_plan_vs_fp64).  The plan is built whatever Cout % 4 is (the scalar epilogue is the same code)."""
    from mudiff_hip import ops
    mode = ops.PRO_AFFINE_SILU if form == 'b' else ops.PRO_NONE
    assert ops.conv_prec_supported(ops.View.from_nchw(g(p.x)), p.Cout, mode, ops.PREC_FP8X)
    we = ops.fp8x_weight_exponent(p.w)
    arena = ops.StatsArena(torch.device(DEV))
    out = p.launch(form, ops.PREC_FP8X, arena, w_exp=we)
    y = _result(out).double()
    ref = p.reference(form, torch.float64)
    rms = lambda e: float(e.pow(2).mean().sqrt())      # noqa: E731
    scale = INV_SQRT2 if form == 'b' else 1.0
    conv_rms = rms(p.conv('silu' if form == 'b' else 'none', torch.float64) * scale)
    e8, e32 = rms(y - ref), rms(p.reference(form, torch.float32).double() - ref)
    print(f'{p.tile} {p.B}x{p.H}x{p.W} {p.Cin}->{p.Cout} form {form} fp8x (2^{we}): rms err {e8:.2e} (bar {4e-5 * conv_rms + 1e-6:.2e}), torch fp32 {e32:.2e}; '
          f'max-abs {float((y - ref).abs().max()):.2e}')
    assert e8 <= 4e-5 * conv_rms + 1e-6
    if out.stats is not None:
        _check_stats(out, y, f'{p.tile} form {form} fp8x (of the stored outputs)')


@pytest.mark.parametrize('name,tile', [('8X2', '8X2'), ('16X1', '16X1'), ('MT2', 'MT1')])
def test_fused_skip_conv_at_ragged_sizes(name, tile):
    """mud_conv_args.skip_*: the 3x3 output (with statistics) and the 1x1 skip conv of the raw input, both against fp64 with the bars of
    test_conv_with_fused_skip_conv (1e-4); the skip output is a slice of a wider sentinel-filled buffer.  The third shape takes MT2 as a
    plain launch and MT1 here, at a chip-filling grid."""
    from mudiff_hip import ops
    p = _problem(name, True)
    gen = torch.Generator().manual_seed(p.Cin + p.Cout)
    w2, bias_s = torch.randn(p.Cout, p.Cin, 1, 1, generator=gen) / math.sqrt(p.Cin), torch.randn(p.Cout, generator=gen)
    xv = _slice_in(p.x)
    assert ops.fused_skip_ok(xv, p.Cout, ops.PRO_AFFINE_SILU)
    assert ops.TILE_NAMES[ops.conv_tile(xv, p.Cout, skip=True)] == tile and ops.TILE_NAMES[ops.conv_tile(xv, p.Cout)] == p.tile
    arena = ops.StatsArena(torch.device(DEV))
    out, skip = _slice_out(p.B, p.H, p.W, p.Cout, arena), _slice_out(p.B, p.H, p.W, p.Cout)
    ops.conv(xv, ops.pack_conv_weight(g(p.w)), 3, p.Cout, mfma=True, pro=(g(p.sc), g(p.sh), ops.PRO_AFFINE_SILU), bias=g(p.bias), bias2=g(p.bias2), out=out,
             skip=(ops.pack_conv_weight(g(w2)), g(bias_s), skip))
    ref = p.conv('silu', torch.float64) + p.bias.double()[None, :, None, None] + p.bias2.double()[:, :, None, None]
    ref_s = F.conv2d(p.x.double(), w2.double(), bias_s.double())
    r32 = p.conv('silu', torch.float32) + p.bias[None, :, None, None] + p.bias2[:, :, None, None]
    e1, e2 = float((_result(out).double() - ref).abs().max()), float((_result(skip).double() - ref_s).abs().max())
    f1, f2 = float((r32.double() - ref).abs().max()), float((F.conv2d(p.x, w2, bias_s).double() - ref_s).abs().max())
    print(f'fused skip conv on {tile} {p.B}x{p.H}x{p.W} {p.Cin}->{p.Cout}: 3x3 {e1:.2e} (torch fp32 {f1:.2e}), 1x1 skip {e2:.2e} (torch fp32 {f2:.2e}), bar 1e-4')
    assert e1 <= 1e-4 and e2 <= 1e-4
    _check_stats(out, ref, f'fused skip conv on {tile}')


def test_split_k_next_to_a_ragged_tile():
    """(1, 13, 35, 260 -> 68), form b: four K slices of the 17 chunks (cm_splits) on ragged 4-row tiles.  Bit-equal to itself over three
    launches, inside the default plan's bar, and within 2e-5 of the unsplit launch (test_conv_split_k_small_grids)."""
    import mudiff_hip
    from mudiff_hip import ops
    p = Problem('split-K', dims=(1, 13, 35, 260, 68), tile='MT1')
    xv = _slice_in(p.x)
    assert ops.conv3x3_would_split_k(xv, p.Cout) and ops.TILE_NAMES[ops.conv_tile(xv, p.Cout)] == 'MT1'
    arena = ops.StatsArena(torch.device(DEV))
    out = p.launch('b', ops.PREC_16X3, arena)
    # the launch as issued really is split: the wrapper's own query, with this launch's views
    rv = _slice_in(p.res)
    a = mudiff_hip.ConvArgs()
    a.x, a.B, a.H, a.W, a.Cin, a.ldx, a.ks, a.stride, a.pad = xv.ptr, p.B, p.H, p.W, p.Cin, xv.ld, 3, 1, 1
    a.out, a.Cout, a.ldo, a.res, a.ldr = out.ptr, p.Cout, out.ld, rv.ptr, rv.ld
    assert mudiff_hip.load().mud_conv2d_mfma_splitk_bytes(C.byref(a)) == 4 * 16 * 256 * 32 * 4      # 4 slabs x 16 workgroup tiles x 256 threads x 32 words
    y = _result(out)
    tag = f'split-K MT1 {p.B}x{p.H}x{p.W} {p.Cin}->{p.Cout} form b'
    ref = _judge(p, 'b', y, tag)
    _check_stats(out, ref, tag)
    for _ in range(3):                                              # whichever workgroup arrives last, the sum is the same
        assert torch.equal(_result(p.launch('b', ops.PREC_16X3, None)), y)
    assert int(ops.splitk_counters(torch.device(DEV)).abs().sum()) == 0
    y1 = _result(p.launch('b', ops.PREC_16X3, None, split_k=False))
    _judge(p, 'b', y1, tag + ' (unsplit)')
    d = float((y - y1).abs().max())
    print(f'{tag}: split vs unsplit {d:.2e} (bar 2e-5)')
    assert d <= 2e-5


ONE_BY_ONE = [(3, 5, 7, 36, 40), (2, 13, 21, 20, 62)]           # 35 and 273 pixels per image: no multiple of the 128-pixel tile


@functools.lru_cache(maxsize=2)
def _problem_1x1(dims):
    return Problem('1x1', ks=1, dims=dims)


@pytest.mark.parametrize('form', ['a', 'a-contiguous', 'b-affine', 'e', 'e-all', 'f'])
@pytest.mark.parametrize('dims', ONE_BY_ONE, ids=['x'.join(map(str, d)) for d in ONE_BY_ONE])
def test_1x1_kernel_forms(dims, form):
    """k_conv_mfma_regb carries its own copy of the epilogue: bias, prologue + residual + rescale + statistics, sigmoid + emul (on some
    / on all channels) and the gated mix, on the vector (Cout = 40) and the scalar (Cout = 62) path."""
    from mudiff_hip import ops
    p = _problem_1x1(dims)
    arena = ops.StatsArena(torch.device(DEV))
    out = p.launch(form, ops.PREC_16X3, arena)
    ref = _judge(p, form, _result(out), f'1x1 {p.B}x{p.H}x{p.W} {p.Cin}->{p.Cout} form {form}')
    if out.stats is not None:
        _check_stats(out, ref, f'1x1 form {form}')


@pytest.mark.parametrize('dims', ONE_BY_ONE, ids=['x'.join(map(str, d)) for d in ONE_BY_ONE])
def test_1x1_kernel_per_sample_weights(dims):
    """w_bstride: one weight matrix per sample (the packing of the unfused attention path: pack_weights(nbatch = B)), with out_scale."""
    from mudiff_hip import ops
    p = _problem_1x1(dims)
    gen = torch.Generator().manual_seed(p.Cin * p.Cout)
    wb = torch.randn(p.B, p.Cout, p.Cin, generator=gen) / math.sqrt(p.Cin)
    wp = ops.pack_weights(g(wb), 0, 1, p.Cin, 1, p.Cin, p.Cout, nbatch=p.B, src_bstride=p.Cout * p.Cin)
    out = _slice_out(p.B, p.H, p.W, p.Cout)
    ops.conv(_slice_in(p.x), wp, 1, p.Cout, mfma=True, out_scale=0.25, out=out, w_bstride=wp.shape[1])
    ref = torch.einsum('boi,bihw->bohw', wb.double(), p.x.double()) * 0.25
    err = float((_result(out).double() - ref).abs().max())
    e32 = float((torch.einsum('boi,bihw->bohw', wb, p.x).double() * 0.25 - ref).abs().max())
    bar = 3e-5 * max(1.0, float(ref.abs().max()))
    print(f'1x1 {p.B}x{p.H}x{p.W} {p.Cin}->{p.Cout} per-sample weights: max-abs vs fp64 {err:.2e} (bar {bar:.2e}), torch fp32 {e32:.2e}')
    assert err <= bar
