"""Tensor-level wrappers over the C ABI: NHWC views, shape checks on the host, launches on torch's
current stream.  Everything here is GPU-only (see mudiff_hip.__init__)."""
from __future__ import annotations

import collections
import ctypes as C
import math
import os

import numpy as np
import torch

from . import (ACT_LRELU, ACT_NONE, ACT_SIGMOID, ACT_SILU, ACT_TANH, PREC_16X1, PREC_16X3, PREC_FP8X, PRO_AFFINE, PRO_AFFINE_SILU, PRO_LRELU,  # noqa: F401
               PRO_NONE, TILE_8X1R, TILE_8X2, TILE_16X1, TILE_MT1, TILE_MT2, ConvArgs, MudiffHipError, check, load, ptr, require_gpu)


# MUD_DETERMINISTIC=1: bit-stable outputs run to run.  The only order-dependent arithmetic of the path is the fp64 atomic
# accumulation of the GroupNorm (sum, sumsq) in the producers' epilogues (~1e-6 jitter on the outputs); with this switch the
# producers accumulate nothing and every GroupNorm re-reads its input with per-workgroup partials + a fixed-order finalize
# (mud_gn_scale_shift).  The reference's CPU path is deterministic; this costs one extra pass over each normalised tensor.
DETERMINISTIC = os.environ.get('MUD_DETERMINISTIC', '0') == '1'


class StatsArena:
    """Zeroed fp64 scratch for the per-(sample, channel) (sum, sumsq) accumulators that producers fill in
    their epilogues for the next GroupNorm.  One memset per chunk instead of one per tensor."""

    def __init__(self, device, chunk_doubles=1 << 18):
        self.device, self.chunk = device, chunk_doubles
        self.buf, self.used = None, 0

    def take(self, B, C):
        if DETERMINISTIC:         # no producer-side statistics: every GroupNorm takes the fixed-order two-pass reduction
            return None
        n = B * C * 2
        if self.buf is None or self.used + n > self.buf.numel():
            self.buf = torch.zeros(max(self.chunk, n), device=self.device, dtype=torch.float64)
            self.used = 0
        t = self.buf[self.used:self.used + n].view(B, C, 2)
        self.used += n
        return t


class View:
    """NHWC fp32 view (ptr, B, H, W, C, ld) into a torch tensor that owns the memory.  `stats`, when
    present, is a [B, ld, 2] fp64 tensor aligned with the buffer's channel axis that producers of this
    view accumulate per-channel (sum, sum of squares) into (see mud_conv_args.stats)."""
    __slots__ = ('base', 'B', 'H', 'W', 'C', 'ld', 'c0', 'stats')

    def __init__(self, base, B, H, W, C, ld=None, c0=0, stats=None):
        self.base, self.B, self.H, self.W, self.C = base, B, H, W, C
        self.ld = C if ld is None else ld
        self.c0 = c0
        self.stats = stats

    @staticmethod
    def empty(B, H, W, C, device, arena=None):
        v = View(torch.empty(B, H, W, C, device=device, dtype=torch.float32), B, H, W, C)
        if arena is not None:
            v.stats = arena.take(B, C)
        return v

    @property
    def stats_ptr(self):
        return None if self.stats is None else C.c_void_p(self.stats.data_ptr() + 16 * self.c0)

    @staticmethod
    def from_nchw(x):
        """NCHW torch tensor -> NHWC view (zero-copy when C == 1)."""
        require_gpu(x)
        B, Cc, H, W = x.shape
        x = x.float()
        t = x.reshape(B, H, W, 1) if Cc == 1 else x.permute(0, 2, 3, 1)
        return View(t.contiguous(), B, H, W, Cc)

    def to_nchw(self):
        t = self.tensor()
        if self.C == 1:
            return t.reshape(self.B, 1, self.H, self.W)
        return t.permute(0, 3, 1, 2).contiguous()

    def tensor(self):
        """The viewed region as a (possibly non-contiguous) torch tensor [B,H,W,C]."""
        return self.base.reshape(self.B, self.H, self.W, self.ld)[..., self.c0:self.c0 + self.C]

    def up2_shape(self):
        """This view with H and W doubled, for size queries only: the shape a launch that up-samples it on the way in runs at
        (conv(in_up2=...))."""
        return View(self.base, self.B, 2 * self.H, 2 * self.W, self.C, self.ld, self.c0)

    def s2d_shape(self):
        """The 2x2 space-to-depth view of this view, for size queries only: [B, H/2, W/2, 4C], the shape a launch that folds it on
        the way in runs at (conv(in_s2d=True)).  The pointer, ld and c0 stay the full-resolution view's."""
        return View(self.base, self.B, self.H // 2, self.W // 2, 4 * self.C, self.ld, self.c0)

    def slice(self, c0, C_):
        assert 0 <= c0 and c0 + C_ <= self.C
        return View(self.base, self.B, self.H, self.W, C_, self.ld, self.c0 + c0, self.stats)

    @property
    def ptr(self):
        return C.c_void_p(self.base.data_ptr() + 4 * self.c0)

    @property
    def npix(self):
        return self.B * self.H * self.W

    @property
    def device(self):
        return self.base.device


class _Profile:
    """Optional per-launch timing with HIP events on the launching stream (bench.py's roofline leg)."""

    def __init__(self):
        self.on = False
        self.records = []

    def enable(self):
        self.on, self.records = True, []

    def disable(self):
        self.on = False

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1, flops, nbytes in self.records:
            d = out.setdefault(name, dict(n=0, ms=0.0, flops=0.0, bytes=0.0))
            d['n'] += 1
            d['ms'] += e0.elapsed_time(e1)
            d['flops'] += flops
            d['bytes'] += nbytes
        return out


PROFILE = _Profile()


STREAM = object()      # placeholder argument: replaced by the launch device's current HIP stream


def _launch(name, dev, fn, *args, flops=0.0, nbytes=0.0):
    """Enqueue one C-ABI call on the current stream of `dev` - the device the operands live on, which need not be the
    process's current device (the kernels take raw pointers: a launch on another device would fault or silently run on
    the wrong GPU)."""
    idx = torch.cuda.current_device() if dev.index is None else dev.index
    if idx != torch.cuda.current_device():
        with torch.cuda.device(idx):
            return _launch(name, dev, fn, *args, flops=flops, nbytes=nbytes)
    args = tuple(C.c_void_p(torch.cuda.current_stream().cuda_stream) if a_ is STREAM else a_ for a_ in args)
    if PROFILE.on:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        code = fn(*args)
        e1.record()
        PROFILE.records.append((name, e0, e1, flops, nbytes))
    else:
        code = fn(*args)
    check(code, name)


def _f32(t):
    assert t.dtype == torch.float32 and t.is_contiguous(), (t.dtype, t.is_contiguous())
    return t


# ---------------------------------------------------------------------------------------------------
def posterior_sample(x01, x02, xt, noise, t, coef1, coef2, std_tab, out=None):
    require_gpu(x01, xt, noise, t, coef1)
    B = xt.shape[0]
    per = xt[0].numel() if B else 0
    x01, xt, noise = _f32(x01.contiguous()), _f32(xt.contiguous()), _f32(noise.contiguous())
    if x02 is not None:
        x02 = _f32(x02.contiguous())
        assert x02.shape == xt.shape
    assert x01.shape == xt.shape == noise.shape and t.dtype == torch.int64 and t.numel() == B
    out = torch.empty_like(xt) if out is None else out
    _launch('posterior_sample', xt.device, load().mud_posterior_sample, ptr(x01), ptr(x02), ptr(xt), ptr(noise), ptr(t.contiguous()), ptr(coef1), ptr(coef2),
                                      ptr(std_tab), coef1.numel(), ptr(out), B, per, STREAM)
    return out


def q_sample(x, noise, t, toff, a_tab, s_tab):
    require_gpu(x, noise, t, a_tab, s_tab)
    x, noise = _f32(x.contiguous()), _f32(noise.contiguous())
    B = x.shape[0]
    out = torch.empty_like(x)
    _launch('q_sample', x.device, load().mud_q_sample, ptr(x), ptr(noise), ptr(t.contiguous()), toff, ptr(a_tab), ptr(s_tab), a_tab.numel(), ptr(out), B,
                              x[0].numel() if B else 0, STREAM)
    return out


def timestep_embedding(t, dim, max_positions=10000.0):
    require_gpu(t)
    assert t.dim() == 1 and t.dtype == torch.int64
    out = torch.empty(t.shape[0], dim, device=t.device, dtype=torch.float32)
    _launch('timestep_embedding', t.device, load().mud_timestep_embedding, ptr(t.contiguous()), ptr(out), t.shape[0], dim, float(max_positions), STREAM)
    return out


def fourier_embedding(t, W):
    """[sin | cos](2*pi*W*log(t)) -> [B, 2*len(W)] (GaussianFourierProjection of log(time_cond))."""
    require_gpu(t, W)
    tf, Wf = _f32(t.float().contiguous()), _f32(W.detach().float().contiguous())
    out = torch.empty(tf.shape[0], 2 * Wf.shape[0], device=t.device, dtype=torch.float32)
    _launch('fourier_embedding', t.device, load().mud_fourier_embedding, ptr(tf), ptr(Wf), ptr(out), tf.shape[0], Wf.shape[0], STREAM)
    return out


def pixel_norm(z):
    require_gpu(z)
    z = _f32(z.contiguous())
    out = torch.empty_like(z)
    _launch('pixel_norm', z.device, load().mud_pixel_norm, ptr(z), ptr(out), z.shape[0], z.shape[1], STREAM)
    return out


def dense(x, W, bias, act_in=ACT_NONE, act_out=ACT_NONE):
    """x [B,K] (row stride allowed), W [N,K], bias [N] -> [B,N]."""
    require_gpu(x, W)
    assert x.dim() == 2 and x.stride(1) == 1 and W.is_contiguous() and x.shape[1] == W.shape[1]
    B, K = x.shape
    N = W.shape[0]
    out = torch.empty(B, N, device=x.device, dtype=torch.float32)
    _launch('dense', x.device, load().mud_dense, ptr(x), x.stride(0) if B > 1 else K, ptr(W), ptr(bias), ptr(out), N, B, K, N, act_in, act_out,
                           STREAM)
    return out


def _mlp_args(a, x, layers, pixel_norm, act, act_last):
    from . import MLP_MAX_LAYERS
    require_gpu(x, *[w for w, _ in layers])
    assert x.dim() == 2 and x.stride(1) == 1 and 1 <= len(layers) <= MLP_MAX_LAYERS
    xin = x if x.dtype == torch.float32 else x.float()
    a.x, a.ldx, a.B, a.nlayers = ptr(xin), (xin.stride(0) if xin.shape[0] > 1 else xin.shape[1]), xin.shape[0], len(layers)
    a.dims[0] = xin.shape[1]
    keep = [xin]
    for l, (w, b) in enumerate(layers):
        w = _f32(w.detach().contiguous())
        assert w.shape[1] == a.dims[l], (tuple(w.shape), a.dims[l])
        a.dims[l + 1] = w.shape[0]
        a.W[l] = w.data_ptr()
        if b is not None:
            b = _f32(b.detach().contiguous())
            a.b[l] = b.data_ptr()
        keep += [w, b]
    a.pixel_norm, a.act, a.act_last = int(pixel_norm), act, int(act_last)
    out = torch.empty(xin.shape[0], a.dims[len(layers)], device=x.device, dtype=torch.float32)
    a.out, a.ldo = ptr(out), out.shape[1]
    return out, keep


def mlp_chain(x, layers, *, pixel_norm=False, act=ACT_SILU, act_last=False):
    """x [B,K0] -> [B,N_last] through `layers` = [(W [N,K], bias [N] or None), ...] in ONE launch (activation between the
    layers, after the last one iff act_last; optional PixelNorm of x first)."""
    return mlp_chains([dict(x=x, layers=layers, pixel_norm=pixel_norm, act=act, act_last=act_last)])[0]


def mlp_chains(chains):
    """Up to four independent chains (dicts of mlp_chain's arguments) side by side in ONE launch -> list of outputs."""
    from . import MlpArgs
    assert 1 <= len(chains) <= 4
    arr = (MlpArgs * len(chains))()
    outs, keep = [], []
    for a, c in zip(arr, chains):
        o, k = _mlp_args(a, c['x'], c['layers'], c.get('pixel_norm', False), c.get('act', ACT_SILU), c.get('act_last', False))
        outs.append(o)
        keep.append(k)
    require_gpu(*[c['x'] for c in chains])
    _launch('mlp_chain', chains[0]['x'].device, load().mud_mlp_chains, arr, len(chains), STREAM)
    return outs


_WS = {}


def _workspace(device, nbytes):
    ws = _WS.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), device=device, dtype=torch.uint8)
        _WS[device] = ws
    return ws


def gn_scale_shift(x: View, G, gamma=None, beta=None, eps=1e-6):
    """-> (scale [B,C], shift [B,C]).  gamma/beta: None, [C] or [B,C] (row-strided views allowed)."""
    lib = load()
    HW = x.H * x.W
    ss = torch.empty(2, x.B, x.C, device=x.device, dtype=torch.float32)
    bstride = 0
    if gamma is not None:
        assert gamma.stride(-1) == 1 and beta.stride(-1) == 1 and gamma.shape[-1] == x.C
        if gamma.dim() == 2:
            assert gamma.shape[0] == x.B and gamma.stride(0) == beta.stride(0)
            bstride = gamma.stride(0)
    if x.stats is not None:      # the producers already accumulated (sum, sumsq): no pass over the tensor
        _launch('gn_from_sums', x.device, lib.mud_gn_scale_shift_from_sums, x.stats_ptr, x.stats.shape[1], x.B, x.C, G, float(HW), eps, ptr(gamma),
                ptr(beta), bstride, ptr(ss[0]), ptr(ss[1]), x.C, STREAM)
        return ss[0], ss[1]
    ws = _workspace(x.device, lib.mud_gn_ws_bytes(x.B, HW, x.C, G))
    _launch('gn_scale_shift', x.device, lib.mud_gn_scale_shift, x.ptr, x.B, HW, x.C, x.ld, G, eps, ptr(gamma), ptr(beta), bstride, ptr(ss[0]),
            ptr(ss[1]), x.C, None, ptr(ws), STREAM, nbytes=4.0 * x.npix * x.C)
    return ss[0], ss[1]


class LazyGN:
    """GroupNorm scale / shift of a view whose producers already accumulated the per-channel (sum, sumsq): nothing is
    launched for it.  A consumer that can finalise it in its own prologue (mud_conv2d_mfma: mud_conv_args.gn_*) takes it as
    `pro=(lazy, None, mode)`; any other consumer calls `.tensors()` (one small launch, cached)."""
    __slots__ = ('x', 'G', 'gamma', 'beta', 'bstride', 'eps', '_ss')

    def __init__(self, x: View, G, gamma, beta, bstride, eps):
        self.x, self.G, self.gamma, self.beta, self.bstride, self.eps, self._ss = x, G, gamma, beta, bstride, eps, None

    def tensors(self):
        if self._ss is None:
            x = self.x
            ss = torch.empty(2, x.B, x.C, device=x.device, dtype=torch.float32)
            _launch('gn_from_sums', x.device, load().mud_gn_scale_shift_from_sums, x.stats_ptr, x.stats.shape[1], x.B, x.C, self.G,
                    float(x.H * x.W), self.eps, ptr(self.gamma), ptr(self.beta), self.bstride, ptr(ss[0]), ptr(ss[1]), x.C, STREAM)
            self._ss = (ss[0], ss[1])
        return self._ss

    def __iter__(self):          # `sc, sh = ...` keeps working for callers that need the arrays
        return iter(self.tensors())


def gn_lazy(x: View, G, gamma=None, beta=None, eps=1e-6):
    """gn_scale_shift whose finalisation is deferred to the consumer when the producers left (sum, sumsq) behind
    (-> LazyGN); otherwise the two-pass statistics run now (-> (scale, shift))."""
    if x.stats is None or not FOLD_GN:
        return gn_scale_shift(x, G, gamma, beta, eps)
    bstride = 0
    if gamma is not None:
        assert gamma.stride(-1) == 1 and beta.stride(-1) == 1 and gamma.shape[-1] == x.C
        if gamma.dim() == 2:
            assert gamma.shape[0] == x.B and gamma.stride(0) == beta.stride(0)
            bstride = gamma.stride(0)
    return LazyGN(x, G, gamma, beta, bstride, eps)


FOLD_GN = os.environ.get('MUD_FOLD_GN', '1') != '0'      # A/B knob: 0 = one gn_from_sums launch per GroupNorm (round-1 behaviour)


FUSE_SKIP = os.environ.get('MUD_FUSE_SKIP', '1') != '0'     # A/B knob: 0 = the 1x1 skip conv stays its own launch (round-1 behaviour)


_SPLITK_COUNTERS = {}
_SPLITK_OWNED = []        # innermost `own_splitk_counters` buffer, if any


def new_splitk_counters(device):
    return torch.zeros(4096, device=device, dtype=torch.int32)


class own_splitk_counters:
    """Context: the split-K launches issued inside use THIS counter array.  A captured hipGraph can be replayed on any stream, and
    two graphs replayed concurrently (two samplers on two streams) must not share arrival counters - a tile would be reduced early
    or never - so every GraphSampler captures with an array of its own instead of the per-(device, stream) one below."""

    def __init__(self, buf):
        self.buf = buf

    def __enter__(self):
        _SPLITK_OWNED.append(self.buf)
        return self.buf

    def __exit__(self, *exc):
        _SPLITK_OWNED.pop()
        return False


def splitk_counters(device):
    """Arrival counters of the in-launch split-K reduction (mud_conv_args.splitk_counters): the array of the enclosing
    `own_splitk_counters` context (graph capture), else one zeroed array per (device, stream) - launches on one stream are ordered,
    and every launch leaves the counters at zero."""
    if _SPLITK_OWNED and _SPLITK_OWNED[-1].device == torch.device(device):
        return _SPLITK_OWNED[-1]
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    buf = _SPLITK_COUNTERS.get(key)
    if buf is None:
        buf = _SPLITK_COUNTERS[key] = new_splitk_counters(device)
    return buf


def _query_args(B, H, W, cin, ld, cout, at=None, skip=False, **fields):
    """The ConvArgs of a 3x3 launch [B,H,W,cin] (row stride ld) -> cout for the library's host-side queries (mud_conv2d_mfma_tile,
    *_supported, _splitk_bytes): only sizes and alignment are looked at, so `at` (a device pointer or None) stands for every operand."""
    a = ConvArgs()
    a.x, a.B, a.H, a.W, a.Cin, a.ldx, a.ks, a.stride, a.pad = at, B, H, W, cin, ld, 3, 1, 1
    a.out, a.Cout, a.ldo = at, cout, (cout + 3) & ~3
    if skip:
        a.skip_w = at
    for name, value in fields.items():
        setattr(a, name, value)
    return C.byref(a)


def conv3x3_would_split_k(x: View, cout):
    """Would mud_conv2d_mfma deal the K chunks of this 3x3 launch to several workgroups (small grid, long reduction)?"""
    return load().mud_conv2d_mfma_splitk_bytes(_query_args(x.B, x.H, x.W, x.C, x.ld, cout, x.ptr)) > 0


FUSE_SKIP_SPLIT = os.environ.get('MUD_FUSE_SKIP_SPLIT', '1') != '0'       # A/B knob: keep the skip conv fused where the launch is split over K


def fused_skip_ok(x: View, cout, pro_mode):
    """Should mud_conv2d_mfma produce the block's 1x1 skip conv alongside its 3x3 conv (mud_conv_args.skip_*)?  Where the launch
    is split over K (one slice at a time, 64x64 maps) the fused kernel splits too - both accumulator sets go through the slabs and
    the last workgroup of a tile reduces them (an unsplit fused launch there cost 109 us against 59 + 23 us: 512->256)."""
    return (FUSE_SKIP and pro_mode == PRO_AFFINE_SILU and x.C % 4 == 0 and 8 <= x.C <= 512 and cout % 4 == 0
            and (FUSE_SKIP_SPLIT or not conv3x3_would_split_k(x, cout)))


RES_UP2 = os.environ.get('MUD_RES_UP2', '1') != '0'     # A/B knob: 0 = the up blocks' skip path is up-sampled by a FIR launch of its own


def up2_taps(kernel2d, up, down, pad):
    """The four 1-D taps t (gain included) of an x2 up-sampling FIR whose 4x4 kernel is exactly t (x) t with pad (2, 1) - the form
    mud_conv_args.res_up2 takes - or None for any other filter."""
    k = np.asarray(kernel2d, dtype=np.float32)
    if k.shape != (4, 4) or (up, down, tuple(pad)) != (2, 1, (2, 1)) or not float(k.sum()) > 0.0:
        return None
    t = (k.sum(axis=1) / np.sqrt(k.sum())).astype(np.float32)
    return tuple(float(v) for v in t) if np.array_equal(np.outer(t, t).astype(np.float32), k) else None


def res_up2_ok(B, H, W, cin, cout):
    """Does a 3x3 mud_conv2d_mfma launch of these sizes ([B,H,W,cin] -> cout) take its residual up-sampled on load
    (mud_conv2d_mfma_res_up2_supported: the AdaGN + SiLU prologue, even H and W, a grid that is not split over K)?"""
    if not RES_UP2 or cin % 4 or cout % 4:
        return False
    return bool(load().mud_conv2d_mfma_res_up2_supported(_query_args(B, H, W, cin, cin, cout, pro_mode=PRO_AFFINE_SILU)))


IN_UP2 = os.environ.get('MUD_IN_UP2', '1') != '0'       # A/B knob: 0 = the up blocks' Conv_0 reads a tensor that a FIR launch of its own up-sampled


def in_up2_ok(B, H, W, cin, cout, prec=PREC_16X3):
    """Does a 3x3 mud_conv2d_mfma launch with OUTPUT size [B,H,W,cout] under plan `prec` take its input [B,H/2,W/2,cin] up-sampled
    while it is staged (mud_conv2d_mfma_in_up2_supported: the AdaGN + SiLU prologue, even H and W, a tile and plan the form is built
    for, a grid that is not split over K)?  Independent of RES_UP2."""
    if not IN_UP2 or cin % 4 or cout % 4:
        return False
    return bool(load().mud_conv2d_mfma_in_up2_supported(_query_args(B, H, W, cin, cin, cout, pro_mode=PRO_AFFINE_SILU, prec=prec)))


PYR_S2D = os.environ.get('MUD_PYR_S2D', '1') != '0'     # A/B knob: 0 = the input pyramid's down-sampler runs its FIR launch and the sub2 conv launch


def in_s2d_ok(B, H, W, c, cout, prec=PREC_16X3):
    """Does a 3x3 mud_conv2d_mfma launch under plan `prec` take the FULL-resolution input [B,H,W,c] as its 2x2 space-to-depth view
    [B,H/2,W/2,4c], gathered while it is staged (mud_conv2d_mfma_in_s2d_supported: no prologue, c % 16 == 0, a tile and plan the form
    is built for, a grid that is not split over K)?  The PYR_S2D knob is the dispatcher's (up_or_down_sampling.padded_strided_conv)."""
    if H % 2 or W % 2 or c % 16 or cout % 4:
        return False
    return bool(load().mud_conv2d_mfma_in_s2d_supported(_query_args(B, H // 2, W // 2, 4 * c, c, cout, pro_mode=PRO_NONE, prec=prec, in_s2d=1)))


def s2d_fold(t):
    """[B,H,W,C] -> the materialised 2x2 space-to-depth tensor [B,H/2,W/2,4C] in mud_conv_args.in_s2d's channel order
    ((py*2 + px)*C + c); a reference for tests and tools - the launches gather it themselves."""
    B, H, W, Cc = t.shape
    return t.reshape(B, H // 2, 2, W // 2, 2, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4 * Cc).contiguous()


def resolve_pro(pro):
    """(scale, shift, mode) with the arrays materialised (for consumers that cannot fold the GroupNorm finalisation)."""
    if pro is not None and isinstance(pro[0], LazyGN):
        sc, sh = pro[0].tensors()
        return (sc, sh, pro[2])
    return pro


def channel_mean(x: View):
    lib = load()
    HW = x.H * x.W
    ws = _workspace(x.device, lib.mud_gn_ws_bytes(x.B, HW, x.C, x.C))
    out = torch.empty(x.B, x.C, device=x.device, dtype=torch.float32)
    _launch('channel_mean', x.device, lib.mud_channel_mean, x.ptr, x.B, HW, x.C, x.ld, ptr(out), x.C, ptr(ws), STREAM, nbytes=4.0 * x.npix * x.C)
    return out


# ---------------------------------------------------------------------------------------------------
def pack_weights(src, s_tap, s_ci, s_co, ks, Cin, Cout, nbatch=1, src_bstride=0, src_offset=0, prec=PREC_16X3, w_exp=0):
    """-> uint8 tensor [nbatch, packed bytes] in the MFMA kernel's B-operand layout (for the arithmetic plan `prec`)."""
    lib = load()
    require_gpu(src)
    nbytes = lib.mud_packed_weight_bytes_prec(ks, Cin, Cout, prec)
    if nbytes < 0:
        raise MudiffHipError(f'pack_weights: plan {prec} has no packed form for ks={ks}')
    dst = torch.empty(nbatch, nbytes, device=src.device, dtype=torch.uint8)
    _launch('pack_weights', src.device, lib.mud_pack_weights_prec, C.c_void_p(src.data_ptr() + 4 * src_offset), s_tap, s_ci, s_co, src_bstride, ks, Cin, Cout,
            nbatch, prec, w_exp, ptr(dst), STREAM)
    return dst


def fp8x_weight_exponent(w):
    """The power-of-two pre-scale of a layer's e4m3 weight image (MUD_PREC_FP8X): the largest e with max|w| * 2^e <= 448 (e4m3's
    largest finite value), so that the 4 significant bits sit where this layer's weights are.  Host sync: pack time only."""
    m = float(w.detach().abs().max())
    if not (m > 0.0) or not math.isfinite(m):
        return 0
    return max(-100, min(100, int(math.floor(math.log2(448.0 / m)))))


def pack_conv_weight(w_oihw, prec=PREC_16X3, w_exp=0):
    """nn.Conv2d weight [O,I,k,k] -> packed MFMA operand."""
    O, I, k, _ = w_oihw.shape
    w = _f32(w_oihw.detach().contiguous())
    return pack_weights(w, 1, k * k, I * k * k, k, I, O, prec=prec, w_exp=w_exp)


def pack_matrix_in_out(W_in_out):
    """NIN weight W[in,out] -> packed 1x1 operand."""
    I, O = W_in_out.shape
    return pack_weights(_f32(W_in_out.detach().contiguous()), 0, O, 1, 1, I, O)


def direct_weight(w_oihw):
    """[O,I,k,k] -> fp32 [k,k,I,O] for mud_conv2d_direct."""
    return w_oihw.detach().permute(2, 3, 1, 0).contiguous()


# ---- arithmetic plan per 3x3 launch (mud_conv_args.prec).  MUD_PREC_PLAN: 'auto' (default) = the fp16 + e4m3-cross-term plan
# (MUD_PREC_FP8X) for every launch the library has it for (fp8x_pays), fp16 x 3 elsewhere (small grids, 1x1, the exact head / tail
# kernels); 'off' = every launch fp16 x 3; 'all' = wherever the library has the plan, whatever fp8x_pays says; 'fp16' = the
# single-pass plan (MUD_PREC_16X1: fp16 operands, fp32 accumulation - autocast's arithmetic, NOT the parity plan) on every 3x3
# launch of the generators, fp16 x 3 elsewhere (1x1 GEMMs, attention, the critic, the exact direct kernels).
PREC_PLAN = os.environ.get('MUD_PREC_PLAN', 'auto')


def fp8x_pays(B, H, W, cin, cout):
    """Should a launch the library has MUD_PREC_FP8X for take it?  Per launch in isolation (scripts/ab_prec.py, batch 16,
    profiles/r03_g_ab_prec_b16.txt) the plan is 0.86-0.99x of the fp16 x 3 launch on every shape it is built for (the 64 -> 64
    layers at 256x256 included, on their one-row tile), and the whole bench line alternated on one box agrees
    (profiles/r03_d_plan_alternation.txt): no shape is excluded.  The hook stays for shapes a later measurement finds to lose."""
    return True


PREC_PLANS = ('off', 'auto', 'all', 'fp16')


class prec_plan:
    """Context: PREC_PLAN = `name` ('off' | 'auto' | 'all' | 'fp16') for the launches planned inside (eager calls; a graph captured
    inside keeps the plans it was captured with), restored on exit."""

    def __init__(self, name):
        if name not in PREC_PLANS:
            raise ValueError(f'prec_plan: unknown plan {name!r} (one of {PREC_PLANS})')
        self.name, self._saved = name, None

    def __enter__(self):
        global PREC_PLAN
        self._saved, PREC_PLAN = PREC_PLAN, self.name
        return self

    def __exit__(self, *exc):
        global PREC_PLAN
        PREC_PLAN = self._saved
        return False


def conv_prec_supported(x: View, cout, pro_mode, prec, skip=False, sub2=False):
    """Does mud_conv2d_mfma have plan `prec` for this 3x3 launch (mud_conv2d_mfma_prec_supported)?"""
    return bool(load().mud_conv2d_mfma_prec_supported(_query_args(x.B, x.H, x.W, x.C, x.ld, cout, x.ptr, skip, pro_mode=pro_mode, sub2=int(sub2)), prec))


TILE_NAMES = {TILE_8X2: '8X2', TILE_16X1: '16X1', TILE_MT2: 'MT2', TILE_MT1: 'MT1', TILE_8X1R: '8X1R'}


def conv_tile(x: View, cout, *, skip=False, in_up2=False, in_s2d=False, pro_mode=PRO_NONE, prec=PREC_16X3):
    """The workgroup tile (TILE_*) a 3x3 mud_conv2d_mfma launch of this shape runs on (mud_conv2d_mfma_tile: it follows from the
    workgroup count, not from the layer), or -1 where in_up2 / in_s2d is not built for that tile and plan.  `x`: the view the launch
    reads, as ops.conv takes it (in_up2: the low-resolution view; in_s2d: the full-resolution view).  Only sizes are looked at."""
    if in_up2:
        x = x.up2_shape()
    if in_s2d:
        x = x.s2d_shape()
    return load().mud_conv2d_mfma_tile(_query_args(x.B, x.H, x.W, x.C, x.ld, cout, x.ptr, skip, pro_mode=pro_mode, prec=prec, in_up2=int(in_up2),
                                                   in_s2d=int(in_s2d)))


def choose_prec(x: View, cout, pro_mode, *, skip=False, sub2=False, w_bstride=0):
    """The plan a 3x3 mud_conv2d_mfma launch of this shape runs with."""
    if PREC_PLAN == 'off' or w_bstride or x.C % 4:
        return PREC_16X3
    if PREC_PLAN == 'fp16':
        return PREC_16X1 if conv_prec_supported(x, cout, pro_mode, PREC_16X1, skip=skip, sub2=sub2) else PREC_16X3
    if PREC_PLAN != 'all' and not fp8x_pays(x.B, x.H, x.W, x.C, cout):
        return PREC_16X3
    return PREC_FP8X if conv_prec_supported(x, cout, pro_mode, PREC_FP8X, skip=skip, sub2=sub2) else PREC_16X3


# One entry of a launch record (precision.launch_record): layer name (None where no ConvParam names the launch), kernel size,
# matrix-core kernel or not, arithmetic plan, (B, H, W, Cin, Cout), sub2 form, fused skip conv, prologue mode.
# sub2: the launch computes a stride-2 pad-0 convolution on the stride-1 kernel - by the sub2 epilogue (shape: the padded image's) or
# as the folded space-to-depth launch (shape: the folded view's).  Neither is planned by choose_prec: fp16 x 3, or single-pass.
# s2d tells the two apart: True for the folded launch (mud_conv_args.in_s2d), which has no sub2 epilogue.
Launch = collections.namedtuple('Launch', 'layer ks mfma prec shape sub2 skip pro s2d', defaults=(False,))


RECORD = None         # the active precision.launch_record() list, or None: every ops.conv call appends a Launch to it


def conv(x: View, w, ks, Cout, *, mfma, stride=1, pad=None, pro=None, bias=None, bias2=None, res: View = None,
         out_scale=1.0, act=ACT_NONE, out: View = None, w_bstride=0, arena=None, sub2=False, emul: View = None, gate=None, emul_cout=0,
         skip=None, prec=PREC_16X3, w_exp=0, layer=None, res_up2=None, split_k=True, in_up2=None, in_s2d=False, flops=None):
    """One fused convolution launch.  pro = (scale [B,Cin], shift [B,Cin], mode).
    skip = (packed 1x1 weights, bias or None, out View): the same launch also writes the 1x1 convolution of the RAW input
    (the residual block's Conv_2) - see fused_skip_ok().  prec / w_exp: the arithmetic plan `w` was packed for.
    layer: the launch's layer name in a launch record (precision.launch_record).
    res_up2 = the four 1-D taps of a separable 4x4 x2 up-sampling filter (up2_taps): `res` is then the LOW-resolution view
    [B,Ho/2,Wo/2,Cout] and the launch up-samples it while loading it (mud_conv_args.res_up2; see res_up2_ok).
    split_k=False: hand the launch no split-K workspace, so a small grid runs unsplit (a res_up2 launch never gets one).
    in_up2 = the four 1-D taps of such a filter: `x` is then the LOW-resolution view [B,Ho/2,Wo/2,Cin], `pro` the AdaGN + SiLU
    prologue of that view, and the launch convolves FIR x2 (silu(affine(x))), formed while x is staged (mud_conv_args.in_up2; see
    in_up2_ok).  The launch is recorded, and its plan chosen, at the size it runs at: [B,Ho,Wo,Cin].
    in_s2d=True: `x` is the FULL-resolution view [B,2Ho,2Wo,Cin/4] and the launch convolves its 2x2 space-to-depth view
    [B,Ho,Wo,Cin] (channel (py*2 + px)*C + c), gathered while x is staged; `w` is packed for that view (mud_conv_args.in_s2d; see
    in_s2d_ok).  Recorded at the size it runs at.  flops: the algorithmic count to book instead of the launch's own (a launch that
    stands for another operator, e.g. a folded stride-2 convolution)."""
    if in_s2d:
        assert mfma and ks == 3 and stride == 1 and not sub2 and skip is None and res_up2 is None and in_up2 is None and pro is None
        if x.H % 2 or x.W % 2 or x.C % 16:
            raise MudiffHipError(f'conv: in_s2d needs even H, W and C % 16 == 0 (got {x.H}x{x.W}, C={x.C})')
        x = x.s2d_shape()                         # (sizes below are the launch's; the pointer and ld are the full-resolution view's)
    if in_up2 is not None:
        assert mfma and ks == 3 and stride == 1 and not sub2 and skip is None and res_up2 is None and len(in_up2) == 4
        assert pro is not None and pro[2] == PRO_AFFINE_SILU
        x_lo, x = x, x.up2_shape()                # (sizes below are the launch's; the pointer and the statistics are the low-resolution view's)
    if RECORD is not None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('precision.launch_record() is eager only: the launch is being captured into a graph')
        RECORD.append(Launch(layer, ks, bool(mfma), prec, (x.B, x.H, x.W, x.C, Cout), bool(sub2 or in_s2d), skip is not None,
                             PRO_NONE if pro is None else pro[2], bool(in_s2d)))
    lib = load()
    pad = ks // 2 if pad is None else pad
    Ho = (x.H + 2 * pad - ks) // stride + 1
    Wo = (x.W + 2 * pad - ks) // stride + 1
    if sub2:      # stride-2 pad-0 result obtained from the stride-1 pad-1 kernel by keeping odd positions
        assert mfma and ks == 3 and stride == 1 and x.H % 2 == 1 and x.W % 2 == 1
        Ho, Wo = x.H // 2, x.W // 2
    if out is None:
        out = View.empty(x.B, Ho, Wo, Cout, x.device, arena)
    assert (out.B, out.H, out.W, out.C) == (x.B, Ho, Wo, Cout), ((out.B, out.H, out.W, out.C), (x.B, Ho, Wo, Cout))
    a = ConvArgs()
    a.x, a.B, a.H, a.W, a.Cin, a.ldx = x.ptr, x.B, x.H, x.W, x.C, x.ld
    a.w, a.w_bstride = ptr(w), w_bstride
    a.ks, a.stride, a.pad = ks, stride, pad
    keep = None          # tensors the launch reads that nothing else references (lazy GroupNorm operands, split-K slabs)
    if pro is not None and isinstance(pro[0], LazyGN) and not (mfma and x.C <= 1024 and pro[0].x.stats is not None):
        pro = resolve_pro(pro)
    if pro is not None and pro[2] == PRO_LRELU:
        a.pro_mode = PRO_LRELU
    elif pro is not None and isinstance(pro[0], LazyGN):      # finalised inside the kernel's prologue
        gn = keep = pro[0]
        assert gn.x.C == x.C and gn.x.B == x.B
        a.pro_mode = pro[2]
        a.gn_sums, a.gn_sums_ld, a.gn_G, a.gn_eps, a.gn_count = gn.x.stats_ptr, gn.x.stats.shape[1], gn.G, gn.eps, float(gn.x.H * gn.x.W)
        a.gn_gamma, a.gn_beta, a.gn_bstride = ptr(gn.gamma), ptr(gn.beta), gn.bstride
    elif pro is not None:
        sc, sh, mode = pro
        assert sc.shape == (x.B, x.C) and sc.stride(1) == 1 and sh.stride() == sc.stride()
        a.pro_scale, a.pro_shift, a.pro_ld, a.pro_mode = ptr(sc), ptr(sh), sc.stride(0), mode
    else:
        a.pro_mode = PRO_NONE
    if bias is not None:
        assert bias.numel() == Cout and bias.is_contiguous()
        a.bias = ptr(bias)
    if bias2 is not None:
        assert bias2.shape == (x.B, Cout) and bias2.stride(1) == 1
        a.bias2, a.bias2_ld = ptr(bias2), bias2.stride(0)
    if res is not None:
        if res_up2 is not None:
            assert mfma and Ho % 2 == 0 and Wo % 2 == 0 and (res.B, res.H, res.W, res.C) == (x.B, Ho // 2, Wo // 2, Cout) and len(res_up2) == 4
            a.res_up2, a.res_k = 1, (C.c_float * 4)(*res_up2)
        else:
            assert (res.B, res.H, res.W, res.C) == (x.B, Ho, Wo, Cout)
        a.res, a.ldr = res.ptr, res.ld
    if in_up2 is not None:
        a.in_up2, a.in_k = 1, (C.c_float * 4)(*in_up2)
    if in_s2d:
        a.in_s2d = 1
    a.out_scale, a.act = out_scale, act
    a.sub2 = 1 if sub2 else 0
    if emul is not None:          # v *= emul (on the first emul_cout output channels only, when given)
        assert (emul.B, emul.H, emul.W, emul.C) == (x.B, Ho, Wo, emul_cout or Cout)
        a.emul, a.ld_emul, a.emul_cout = emul.ptr, emul.ld, emul_cout
    if gate is not None:          # v = g*v + (1-g)*other
        gv, ov = gate
        assert (gv.B, gv.H, gv.W, gv.C) == (x.B, Ho, Wo, Cout) == (ov.B, ov.H, ov.W, ov.C)
        a.egate, a.ld_egate, a.eother, a.ld_eother = gv.ptr, gv.ld, ov.ptr, ov.ld
    a.out, a.Cout, a.ldo = out.ptr, Cout, out.ld
    a.prec, a.w_exp = prec, w_exp
    if out.stats is not None:
        a.stats, a.stats_ld = out.stats_ptr, out.stats.shape[1]
    skip_flops = 0.0
    if skip is not None:
        sw, sb, so = skip
        assert mfma and ks == 3 and res is None and (so.B, so.H, so.W, so.C) == (x.B, Ho, Wo, Cout)
        a.skip_w, a.skip_bias, a.skip_out, a.skip_ldo = ptr(sw), ptr(sb), so.ptr, so.ld
        skip_flops = 2.0 * x.B * Ho * Wo * Cout * x.C
    if mfma and ks == 3 and split_k and res_up2 is None and in_up2 is None and not in_s2d:      # small grids (one slice at a time): split-K slabs, stream-ordered scratch (graph-capture safe);
                                                   # a launch that up-samples its residual or its input is never split (no workspace: it runs unsplit)
        cnt = splitk_counters(x.device)
        a.splitk_counters, a.splitk_ncounters = ptr(cnt), cnt.numel()
        nws = lib.mud_conv2d_mfma_splitk_bytes(C.byref(a))
        if nws > 0:
            keep = (keep, torch.empty(nws, device=x.device, dtype=torch.uint8))
            a.splitk_ws, a.splitk_ws_bytes = ptr(keep[1]), nws
    fn = lib.mud_conv2d_mfma if mfma else lib.mud_conv2d_direct
    name = (f'conv_mfma_k{ks}' if mfma else f'conv_direct_k{ks}') + {PREC_FP8X: '_fp8x', PREC_16X1: '_fp16'}.get(prec, '')
    if flops is None:
        flops = 2.0 * x.B * Ho * Wo * Cout * x.C * ks * ks + skip_flops     # algorithmic (sub2 issues 4x this)
    nbytes = 4.0 * ((x_lo if in_up2 is not None else x).npix * x.C + out.npix * Cout * ((2 if res is not None else 1) + (1 if skip is not None else 0))) + (w.numel() * w.element_size() if w_bstride == 0 else x.B * w_bstride)
    _launch(name, x.device, fn, C.byref(a), STREAM, flops=flops, nbytes=nbytes)
    return out


CENSUS_FIELDS = ('n', 'n_over', 'n_under', 'n_fp16_over', 'amax_bits')     # struct mud_census_out, in order


def new_census_slot(device):
    """Zeroed device accumulator of e4m3_census: int64 [5] laid out as struct mud_census_out (CENSUS_FIELDS)."""
    return torch.zeros(len(CENSUS_FIELDS), device=device, dtype=torch.int64)


def e4m3_census(x: View, pro, out):
    """Accumulate the e4m3 range census of a MUD_PREC_FP8X convolution input into `out` (new_census_slot): `x` after the
    prologue `pro` = None | (scale, shift, mode) | (LazyGN, None, mode) - the same prologue the conv is given.  A LazyGN is
    finalised here through LazyGN.tensors() (the arithmetic the conv's folded prologue repeats); the conv itself still takes
    the lazy form, so its launch and outputs do not change."""
    from . import CensusArgs
    require_gpu(x.base, out)
    assert out.dtype == torch.int64 and out.numel() == len(CENSUS_FIELDS) and out.is_contiguous()
    a = CensusArgs()
    a.x, a.B, a.H, a.W, a.C, a.ldx = x.ptr, x.B, x.H, x.W, x.C, x.ld
    if pro is None:
        a.pro_mode = PRO_NONE
    else:
        sc, sh, mode = resolve_pro(pro)
        a.pro_mode = mode
        if mode != PRO_NONE:
            assert sc.shape == (x.B, x.C) and sc.stride(1) == 1 and sh.stride() == sc.stride(), (tuple(sc.shape), sc.stride(), sh.stride())
            a.pro_scale, a.pro_shift, a.pro_ld = ptr(sc), ptr(sh), sc.stride(0)
    _launch('e4m3_census', x.device, load().mud_e4m3_census, C.byref(a), ptr(out), STREAM, nbytes=4.0 * x.npix * x.C)
    return out


# ---------------------------------------------------------------------------------------------------
def upfirdn2d_planes(x, kernel, up, down, pad):
    """The reference's native-op boundary: x [N,C,H,W] (any float dtype is computed in fp32)."""
    require_gpu(x, kernel)
    N, Cc, H, W = x.shape
    xin = _f32(x.float().contiguous())
    k = _f32(kernel.float().contiguous())
    kh, kw = k.shape
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad
    Ho = (H * uy + py0 + py1 - kh) // dy + 1
    Wo = (W * ux + px0 + px1 - kw) // dx + 1
    out = torch.empty(N, Cc, Ho, Wo, device=x.device, dtype=torch.float32)
    _launch('upfirdn2d', x.device, load().mud_upfirdn2d, ptr(xin), N * Cc, H, W, ptr(k), kh, kw, ux, uy, dx, dy, px0, px1, py0, py1, ptr(out), STREAM)
    return out.to(x.dtype)


def fir_nhwc(x: View, kernel2d, up, down, pad, pro=None, want_h=True, want_x=False):
    """kernel2d: host list of lists / numpy [kh,kw].  -> (out_h or None, out_x or None)."""
    import numpy as np
    k = np.ascontiguousarray(kernel2d, dtype=np.float32)
    kh, kw = k.shape
    Ho = (x.H * up + pad[0] + pad[1] - kh) // down + 1
    Wo = (x.W * up + pad[0] + pad[1] - kw) // down + 1
    oh = View.empty(x.B, Ho, Wo, x.C, x.device) if want_h else None
    ox = View.empty(x.B, Ho, Wo, x.C, x.device) if want_x else None
    sc = sh = None
    ld = mode = 0
    if pro is not None:
        sc, sh, mode = resolve_pro(pro)
        ld = sc.stride(0)
    _launch('fir_nhwc', x.device, load().mud_fir_nhwc, x.ptr, x.B, x.H, x.W, x.C, x.ld, k.ctypes.data_as(C.POINTER(C.c_float)), kh, kw, up, down,
            pad[0], pad[1], ptr(sc), ptr(sh), ld, mode, oh.ptr if oh else None, oh.ld if oh else 0, ox.ptr if ox else None,
            ox.ld if ox else 0, STREAM, nbytes=4.0 * x.C * (x.npix + x.B * Ho * Wo * (int(want_h) + int(want_x))))
    return oh, ox


def minibatch_stddev(x: View, group):
    """-> [B] tensor: the critic's minibatch-stddev scalar of every sample's group."""
    out = torch.empty(x.B, device=x.device, dtype=torch.float32)
    _launch('minibatch_stddev', x.device, load().mud_minibatch_stddev, x.ptr, x.B, x.H * x.W, x.C, x.ld, group, ptr(out), STREAM)
    return out


def attention_supported(C_):
    return bool(load().mud_attention_supported(C_))


def attention(qkv: View, C_, scale):
    """qkv: view [B,H,W,3C] (q | k | v, contiguous rows) -> View [B,H,W,C]."""
    assert qkv.C == 3 * C_
    n = qkv.H * qkv.W
    out = View.empty(qkv.B, qkv.H, qkv.W, C_, qkv.device)
    nws = load().mud_attention_ws_bytes(qkv.B, n, C_)        # > 0: few workgroups, the keys are split and merged
    ws = torch.empty(nws // 4, device=qkv.device, dtype=torch.float32) if nws else None
    _launch('attention', qkv.device, load().mud_attention, qkv.ptr, qkv.B, n, C_, qkv.ld, float(scale), out.ptr, out.ld, ptr(ws) if nws else None,
            STREAM, flops=4.0 * qkv.B * n * n * C_)
    return out


def softmax_rows_(s, n):
    """in-place softmax over the last axis of a contiguous [..., n] tensor."""
    rows = s.numel() // n
    _launch('softmax_rows', s.device, load().mud_softmax_rows, ptr(s), rows, n, n, STREAM)
    return s


def mul(a: View, b: View, out: View = None):
    out = View.empty(a.B, a.H, a.W, a.C, a.device) if out is None else out
    _launch('mul', a.device, load().mud_mul, a.ptr, a.ld, b.ptr, b.ld, out.ptr, out.ld, a.npix, a.C, STREAM)
    return out


def gate_mix(g: View, att: View, other: View, out: View):
    _launch('gate_mix', g.device, load().mud_gate_mix, g.ptr, g.ld, att.ptr, att.ld, other.ptr, other.ld, out.ptr, out.ld, g.B, g.H * g.W, g.C,
            out.stats_ptr, out.stats.shape[1] if out.stats is not None else 0, STREAM)
    return out


def resize_bilinear(x, size):
    """x [..., H, W] planes -> [..., Ho, Wo]; `F.interpolate(x, size, mode='bilinear', align_corners=False)` semantics
    (reference engine/test_volume.py:274, engine/train.py:959)."""
    require_gpu(x)
    H, W = x.shape[-2:]
    Ho, Wo = int(size[0]), int(size[1])
    xin = _f32(x.float().contiguous())
    out = torch.empty(*x.shape[:-2], Ho, Wo, device=x.device, dtype=torch.float32)
    _launch('resize_bilinear', x.device, load().mud_resize_bilinear, ptr(xin), xin.numel() // (H * W), H, W, Ho, Wo, ptr(out), STREAM)
    return out


def affine_clamp(x, scale, shift, lo, hi):
    """clamp(x*scale + shift, lo, hi) elementwise (fp32)."""
    require_gpu(x)
    xin = _f32(x.float().contiguous())
    out = torch.empty_like(xin)
    _launch('affine_clamp', x.device, load().mud_affine_clamp, ptr(xin), xin.numel(), float(scale), float(shift), float(lo), float(hi), ptr(out), STREAM)
    return out


def value_range(a, b=None):
    """min and max over every element of the fp32 tensors `a` and `b` (driver: all predictions and all targets of a rank) ->
    fp32 device tensor [min, max]; NaN in both if any input is NaN, +inf / -inf if both are empty.  No synchronisation."""
    require_gpu(a, b)
    ain = _f32(a.contiguous())
    bin_ = None if b is None else _f32(b.contiguous())
    out = torch.empty(2, device=a.device, dtype=torch.float32)
    ws = torch.empty(load().mud_value_range_ws_bytes(), device=a.device, dtype=torch.uint8)
    _launch('value_range', a.device, load().mud_value_range, ptr(ain), ain.numel(), ptr(bin_), 0 if bin_ is None else bin_.numel(),
            ptr(out), ptr(ws), STREAM)
    return out


def quantize_u8(x, gmin, gmax):
    """uint8 image of fp32 `x` with the global range [gmin, gmax] (python floats): bit-identical to
    driver.to_uint8 = clip((x - gmin) / (gmax - gmin) * 255.0, 0, 255).astype(uint8) (reference engine/test.py:386-387).
    As there, gmax <= gmin is NOT remapped here: the caller applies the (0, 1) fallback."""
    require_gpu(x)
    gmin, gmax = float(gmin), float(gmax)
    if not gmax > gmin:
        raise ValueError(f'quantize_u8: empty range [{gmin}, {gmax}] (use the (0, 1) fallback of the driver)')
    xin = _f32(x.contiguous())
    out = torch.empty(xin.shape, device=x.device, dtype=torch.uint8)
    # numpy 2 evaluates the expression in fp32 with weak python scalars: fp32(gmin), and fp32 of the difference taken in double
    _launch('quantize_u8', x.device, load().mud_quantize_u8, ptr(xin), xin.numel(), float(np.float32(gmin)), float(np.float32(gmax - gmin)),
            ptr(out), STREAM)
    return out


def slice_metrics_u8(pred, gt):
    """Per-slice sums of uint8 images [n, H, W] (H, W >= 7) -> (sse int64 [n], sae int64 [n], ssim_sum fp64 [n]) device tensors:
    sum (g-p)^2, sum |g-p| and the sum of the per-pixel SSIM (7x7 window, skimage defaults) over the (H-6)(W-6) interior."""
    require_gpu(pred, gt)
    if pred.dtype != torch.uint8 or gt.dtype != torch.uint8 or pred.dim() != 3 or pred.shape != gt.shape:
        raise MudiffHipError(f'slice_metrics_u8: need two uint8 [n, H, W] tensors of one shape (got {pred.dtype} {tuple(pred.shape)}, '
                             f'{gt.dtype} {tuple(gt.shape)})')
    n, H, W = pred.shape
    if H < 7 or W < 7:
        raise MudiffHipError(f'slice_metrics_u8: slices must be at least 7x7 (the SSIM window), got {H}x{W}')
    pin, gin = pred.contiguous(), gt.contiguous()
    sse = torch.empty(n, device=pred.device, dtype=torch.int64)
    sae = torch.empty(n, device=pred.device, dtype=torch.int64)
    ssim_sum = torch.empty(n, device=pred.device, dtype=torch.float64)
    if n == 0:
        return sse, sae, ssim_sum
    nbytes = load().mud_slice_metrics_ws_bytes(n, H, W)
    ws = torch.empty(nbytes, device=pred.device, dtype=torch.uint8)
    _launch('slice_metrics_u8', pred.device, load().mud_slice_metrics_u8, ptr(pin), ptr(gin), n, H, W, ptr(sse), ptr(sae), ptr(ssim_sum),
            ptr(ws), nbytes, STREAM)
    return sse, sae, ssim_sum


# columns of volume_metrics' sums (include/mudiff_hip.h: MUD_VM_*)
VM_N, VM_SSE, VM_SAE, VM_N_INT, VM_SSIM, VM_SS, VM_SS2, VM_SSE_STD = range(8)
VM_NQ, VM_MAX_REGIONS = 8, 8


def volume_metrics(pred, gt, region, std=None, nreg=VM_MAX_REGIONS):
    """Per-plane, per-region sums of a [Z, X, Y] volume pair (Z, X, Y >= 7; planes contiguous): pred, gt (and std) fp32, region uint8
    (voxel v is in region k < nreg when bit k of region[v] is set) -> device fp64 [Z, nreg, VM_NQ]: voxel count, sum d^2, sum |d|,
    interior voxel count, sum of the 7x7x7 SSIM over the interior (skimage defaults, data_range 1), and with `std` sum s, sum s^2,
    sum s*|d| (zeros without), d = pred - gt in fp64.  Bit-identical run to run.  No synchronisation."""
    require_gpu(pred, gt, region, std)
    ts = [pred, gt] + ([] if std is None else [std])
    if any(t.dtype != torch.float32 for t in ts) or region.dtype != torch.uint8:
        raise MudiffHipError(f'volume_metrics: need fp32 pred / gt{" / std" if std is not None else ""} and a uint8 region '
                             f'(got {", ".join(str(t.dtype) for t in ts)}, {region.dtype})')
    if pred.dim() != 3 or any(t.shape != pred.shape for t in ts + [region]):
        raise MudiffHipError(f'volume_metrics: need [Z, X, Y] tensors of one shape (got {", ".join(str(tuple(t.shape)) for t in ts + [region])})')
    Z, X, Y = pred.shape
    if Z < 7 or X < 7 or Y < 7:
        raise MudiffHipError(f'volume_metrics: volumes must be at least 7x7x7 (the SSIM window), got {Z}x{X}x{Y}')
    if not 1 <= int(nreg) <= VM_MAX_REGIONS:
        raise MudiffHipError(f'volume_metrics: nreg must be in [1, {VM_MAX_REGIONS}] (got {nreg})')
    nreg = int(nreg)
    pin, gin, rin = pred.contiguous(), gt.contiguous(), region.contiguous()
    sin = None if std is None else std.contiguous()
    sums = torch.empty(Z, nreg, VM_NQ, device=pred.device, dtype=torch.float64)
    nbytes = load().mud_volume_metrics_ws_bytes(Z, X, Y, nreg)
    ws = torch.empty(nbytes, device=pred.device, dtype=torch.uint8)
    _launch('volume_metrics', pred.device, load().mud_volume_metrics, ptr(pin), ptr(gin), ptr(rin), ptr(sin), Z, X, Y, nreg, ptr(sums),
            ptr(ws), nbytes, STREAM, nbytes=float(pin.numel()) * (9 + (0 if sin is None else 4)))
    return sums


LPIPS_WS_CAP = 512 << 20      # bytes of workspace per lpips_u8 launch sequence: larger n is split into chunks


def lpips_pack(table, conv_w, conv_b, lin_w):
    """Packed LPIPS-alex weights (mud_lpips_pack) from device fp32 tensors in torch layout: the input table [768], the 5 AlexNet conv
    weights [Cout, Cin, k, k] and biases [Cout], the 5 lin weights [C] -> device uint8 tensor of mud_lpips_packed_bytes()."""
    require_gpu(table, *conv_w, *conv_b, *lin_w)
    table = _f32(table.contiguous())
    conv_w, conv_b, lin_w = ([_f32(t.contiguous()) for t in ts] for ts in (conv_w, conv_b, lin_w))
    packed = torch.empty(load().mud_lpips_packed_bytes(), device=table.device, dtype=torch.uint8)
    arr = lambda ts: (C.c_void_p * 5)(*[ptr(t) for t in ts])       # noqa: E731
    _launch('lpips_pack', table.device, load().mud_lpips_pack, ptr(table), arr(conv_w), arr(conv_b), arr(lin_w), ptr(packed), STREAM)
    return packed


def lpips_u8(pred_u8, gt_u8, net, max_ws_bytes=LPIPS_WS_CAP):
    """LPIPS-alex per tap of uint8 image pairs [n, H, W] (H, W >= 31) with the packed weights of `net` (mudiff_hip.lpips_net.LpipsAlex
    on the images' device) -> device fp64 [n, 5]; LPIPS = the row sum.  Slices go through in chunks whose workspace stays within
    `max_ws_bytes`; a slice's result does not depend on the chunking (or on the other slices of its launch)."""
    require_gpu(pred_u8, gt_u8)
    if pred_u8.dtype != torch.uint8 or gt_u8.dtype != torch.uint8 or pred_u8.dim() != 3 or pred_u8.shape != gt_u8.shape:
        raise MudiffHipError(f'lpips_u8: need two uint8 [n, H, W] tensors of one shape (got {pred_u8.dtype} {tuple(pred_u8.shape)}, '
                             f'{gt_u8.dtype} {tuple(gt_u8.shape)})')
    n, H, W = pred_u8.shape
    if H < 31 or W < 31:
        raise MudiffHipError(f'lpips_u8: slices must be at least 31x31 (AlexNet\'s two pools), got {H}x{W}')
    packed = getattr(net, 'packed', None)
    if packed is None or packed.device != pred_u8.device:
        raise MudiffHipError(f'lpips_u8: the LPIPS weights are not packed on {pred_u8.device} (call net.to(device) first)')
    out = torch.empty(n, 5, device=pred_u8.device, dtype=torch.float64)
    if n == 0:
        return out
    lib = load()
    chunk = max(1, min(n, int(max_ws_bytes) // max(lib.mud_lpips_ws_bytes(1, H, W), 1)))
    nbytes = lib.mud_lpips_ws_bytes(chunk, H, W)
    ws = torch.empty(nbytes, device=pred_u8.device, dtype=torch.uint8)
    pin, gin = pred_u8.contiguous(), gt_u8.contiguous()
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        _launch('lpips_u8', pred_u8.device, lib.mud_lpips_u8, ptr(pin[c0:c0 + m]), ptr(gin[c0:c0 + m]), m, H, W, ptr(packed),
                ptr(out[c0:c0 + m]), ptr(ws), nbytes, STREAM, flops=3.47e9 * m * (H * W / 65536.0))
    return out


def to_range_0_1(x):
    """[-1,1] -> [0,1] with clipping: ((x + 1) / 2).clamp(0, 1) (reference engine/test_volume.py:281)."""
    return affine_clamp(x, 0.5, 0.5, 0.0, 1.0)


INV_SQRT2 = 1.0 / math.sqrt(2.0)


# ---------------------------------------------------------------------------------------------------
# N-sample ensembles (csrc/ensemble.hip, mudiff_hip.ensemble)
KIND_X_INIT, KIND_Z, KIND_NOISE = 0, 1, 2
_MAX_SAMPLE = 1 << 31


def check_keys(keys):
    """(slice, sample) row keys -> an int64 [rows, 2] tensor on the host, refused unless slice >= 0 and 0 <= sample < 2^31.  A device
    tensor is copied to the host for the check (one synchronisation)."""
    k = torch.as_tensor(keys).detach().to('cpu', torch.int64)
    if k.dim() != 2 or k.shape[1] != 2:
        raise MudiffHipError(f'randn_keyed: keys must be [rows, 2] = (slice, sample), got {tuple(k.shape)}')
    if k.numel() and int(k[:, 0].min()) < 0:
        raise MudiffHipError('randn_keyed: slice indices must be >= 0')
    if k.numel() and (int(k[:, 1].min()) < 0 or int(k[:, 1].max()) >= _MAX_SAMPLE):
        raise MudiffHipError('randn_keyed: sample indices must lie in [0, 2^31)')
    return k.contiguous()


def _seed64(seed):
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise MudiffHipError(f'randn_keyed: seed must lie in [0, 2^64), got {seed}')
    return seed


def _draw_args(keys_dev, seed, step, kind):
    """The four arguments that name a keyed draw, in the order every entry takes them."""
    return ptr(keys_dev), C.c_uint64(seed), int(step), int(kind)


def randn_keyed_into(out, keys_dev, seed, step, kind):
    """Unchecked launch of ops.randn_keyed into `out` (fp32, contiguous, [rows, ...]) with keys already through check_keys and on
    out's device (GraphSampler.sample_keyed checks its keys once per batch, not once per draw)."""
    rows = keys_dev.shape[0]
    _launch('randn_keyed', out.device, load().mud_randn_keyed, ptr(out), rows, out.numel() // max(rows, 1), *_draw_args(keys_dev, seed, step, kind),
            STREAM)
    return out


def randn_keyed(rows_keys, row_len, seed, step, kind, out=None):
    """Keyed standard normals: row r of the fp32 result [rows, row_len] is a pure function of (seed, slice, sample, step, kind) with
    rows_keys[r] = (slice, sample) (int64 [rows, 2], host or device): Philox4x64-10 + Box-Muller in fp64 (mud_randn_keyed).  `out`:
    a contiguous fp32 device tensor of rows * row_len elements to fill (any shape); without it the result lands on rows_keys's device
    (or the current one for host keys).  kind: KIND_X_INIT, KIND_Z or KIND_NOISE (or KIND_KSPACE / KIND_THICK / KIND_MULTISLICE /
    KIND_BAND / KIND_LOWRES / KIND_SENSE, to inject what ops.kspace_constrain / ops.slab_constrain / ops.slab_kspace_constrain /
    ops.band_constrain / ops.lowres_constrain / ops.sense_constrain draw; KIND_SENSE_MEAS: the measurement noise of mudiff_hip.sense)."""
    k = check_keys(rows_keys)
    seed = _seed64(seed)
    rows, row_len = k.shape[0], int(row_len)
    if out is None:
        dev = rows_keys.device if isinstance(rows_keys, torch.Tensor) and rows_keys.is_cuda else torch.device('cuda', torch.cuda.current_device())
        out = torch.empty(rows, row_len, device=dev, dtype=torch.float32)
    require_gpu(out)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != rows * row_len:
        raise MudiffHipError(f'randn_keyed: out must be a contiguous fp32 tensor of {rows} x {row_len} elements, got {out.dtype} '
                             f'{tuple(out.shape)}')
    _launch('randn_keyed', out.device, load().mud_randn_keyed, ptr(out), rows, row_len, *_draw_args(k.to(out.device), seed, step, kind), STREAM)
    return out


COUPLING_MAX_RADIUS = 32      # include/mudiff_hip.h: MUD_COUPLING_MAX_RADIUS


def coupling_taps_arg(half_taps, radius):
    """(half_taps, R) -> (the ctypes fp64 array mud_randn_keyed_coupled reads on the host at call time, R), checked."""
    from .slice_coupling import check_coupling
    try:
        half, R = check_coupling((half_taps, radius))
    except ValueError as e:
        raise MudiffHipError(f'randn_keyed_coupled: {e}') from None
    return (C.c_double * (R + 1))(*half.tolist()), R


def randn_keyed_coupled_into(out, keys_dev, seed, step, kind, taps, radius):
    """Unchecked launch of ops.randn_keyed_coupled into `out`, as randn_keyed_into; (taps, radius) from coupling_taps_arg."""
    rows = keys_dev.shape[0]
    _launch('randn_keyed_coupled', out.device, load().mud_randn_keyed_coupled, ptr(out), rows, out.numel() // max(rows, 1),
            *_draw_args(keys_dev, seed, step, kind), taps, int(radius), STREAM)
    return out


def randn_keyed_coupled(rows_keys, row_len, seed, step, kind, half_taps, radius, out=None):
    """Slice-coupled keyed normals (mud_randn_keyed_coupled; mudiff_hip.slice_coupling): row r with key (slice s, sample m) is
    fp32(sum_{j=-R..R} half_taps[|j|] * eta(s + j)) with eta(.) the row ops.randn_keyed gives (slice, m) under the same seed, step and
    kind, summed in fp64 in tap order; s + j wraps modulo 2^64.  Everything else as ops.randn_keyed."""
    k = check_keys(rows_keys)
    seed = _seed64(seed)
    taps, R = coupling_taps_arg(half_taps, radius)
    rows, row_len = k.shape[0], int(row_len)
    if out is None:
        dev = rows_keys.device if isinstance(rows_keys, torch.Tensor) and rows_keys.is_cuda else torch.device('cuda', torch.cuda.current_device())
        out = torch.empty(rows, row_len, device=dev, dtype=torch.float32)
    require_gpu(out)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != rows * row_len:
        raise MudiffHipError(f'randn_keyed_coupled: out must be a contiguous fp32 tensor of {rows} x {row_len} elements, got {out.dtype} '
                             f'{tuple(out.shape)}')
    _launch('randn_keyed_coupled', out.device, load().mud_randn_keyed_coupled, ptr(out), rows, row_len, *_draw_args(k.to(out.device), seed, step, kind),
            taps, R, STREAM)
    return out


# ---------------------------------------------------------------------------------------------------
# sampling with a partly acquired target (csrc/known_region.hip, mudiff_hip.known_region)
KIND_KNOWN, KIND_RENOISE = 3, 4      # the draws of mud_known_constrain: the known region's forward noise, RePaint's one-level re-noising


def _level_and_keys(name, clean, t, a_tab, s_tab, noise, keys, rows, device):
    """What the checked wrappers of the four constraints share -> (t, a_tab, s_tab, the keys on `device` or None): without `clean`, t
    (int64 [rows]) and two fp32 tables of one length, contiguous, and then either `noise` or keys for every row (check_keys)."""
    if clean:
        return t, a_tab, s_tab, None
    if t is None or a_tab is None or s_tab is None or t.dtype != torch.int64 or t.numel() != rows or a_tab.numel() != s_tab.numel():
        raise MudiffHipError(f'{name}: need t (int64 [rows]) and two tables of one length')
    kd = None
    if noise is None:
        if keys is None:
            raise MudiffHipError(f'{name}: pass noise or keys')
        k = check_keys(keys)
        if k.shape[0] != rows:
            raise MudiffHipError(f'{name}: {k.shape[0]} keys for {rows} rows')
        kd = k.to(device)
    return t.contiguous(), _f32(a_tab.contiguous()), _f32(s_tab.contiguous()), kd


def _level_args(noise, keys_dev, seed, step, kind, t, toff, a_tab, s_tab, clean):
    """The eleven arguments of every constraint entry that say at which level, and with which draw (_draw_args' four, spelt out: this
    runs once per launch), the measurement is imposed."""
    return (ptr(noise), ptr(keys_dev), C.c_uint64(seed), int(step), int(kind), ptr(t), int(toff), ptr(a_tab), ptr(s_tab),
            1 if a_tab is None else a_tab.numel(), int(bool(clean)))


def _contiguous_into(name, x, noise, out):
    """`out` must be contiguous -> (x and noise made contiguous, out or a new fp32 tensor of x's shape).  An `out` that is x has passed
    as contiguous, so x is then handed on as it is."""
    if out is not None and not out.is_contiguous():
        raise MudiffHipError(f'{name}: out must be contiguous')
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32) if out is None else out
    return x.contiguous(), None if noise is None else noise.contiguous(), out


def _noise_and_out(name, x, noise, out):
    """What the checked wrappers share for the state x (fp32 [rows, ...]): `noise` and `out`, where given, are fp32 of x's shape, and
    _contiguous_into's rule and result."""
    for what, v in (('noise', noise), ('out', out)):
        if v is not None and (v.dtype != torch.float32 or v.shape != x.shape):
            raise MudiffHipError(f'{name}: {what} must be fp32 of shape {tuple(x.shape)}, got {v.dtype} {tuple(v.shape)}')
    return _contiguous_into(name, x, noise, out)


def known_constrain_into(out, x_new, known, mask, keys_dev, seed, step, kind, t, toff, a_tab, s_tab, clean=False, noise=None):
    """Unchecked launch of mud_known_constrain into `out` (fp32, contiguous, [rows, ...]; may be x_new or known): GraphSampler.sample_keyed
    checks its operands once per batch, not once per step.  keys_dev: through check_keys and on out's device (None with `noise`)."""
    rows = out.shape[0]
    _launch('known_constrain', out.device, load().mud_known_constrain, ptr(x_new), ptr(known), ptr(mask),
            *_level_args(noise, keys_dev, seed, step, kind, t, toff, a_tab, s_tab, clean), ptr(out), rows, out.numel() // max(rows, 1), STREAM,
            nbytes=float(out.numel() * (13 if mask is not None else 8)))
    return out


def known_constrain(x_new, known, mask, t, toff, a_tab, s_tab, *, noise=None, keys=None, seed=0, step=0, kind=KIND_KNOWN, clean=False, out=None):
    """out = mask ? (clean ? known : a_tab[c] * known + s_tab[c] * eta) : x_new per element, c = clamp(t[row] + toff, 0, len(a_tab) - 1)
    (mud_known_constrain): the known part is ops.q_sample's arithmetic bit for bit, the rest x_new's bits; a select, so a NaN of `known`
    outside the mask stays out.  x_new, known: fp32 [rows, ...] of one shape; mask: uint8 of that shape, or None = known everywhere
    (x_new may then be None: a keyed q_sample).  eta: `noise` (fp32, that shape) when given, else the keyed normal ops.randn_keyed gives
    keys[r] = (slice, sample) under (seed, step, kind), drawn in the kernel; kind in [0, 15].  t: int64 [rows]; with `clean` it, the
    tables and the draw are not needed.  out: None (a new tensor), x_new or known (in place) or any contiguous fp32 tensor of the shape."""
    require_gpu(x_new, known, mask, noise, t, a_tab, s_tab, out)
    if known.dtype != torch.float32 or known.dim() < 1 or known.shape[0] < 1 or known[0].numel() < 1:
        raise MudiffHipError(f'known_constrain: known must be a non-empty fp32 [rows, ...] tensor, got {known.dtype} {tuple(known.shape)}')
    rows = known.shape[0]
    for name, v, dt in (('x_new', x_new, torch.float32), ('mask', mask, torch.uint8), ('noise', noise, torch.float32), ('out', out, torch.float32)):
        if v is not None and (v.dtype != dt or v.shape != known.shape):
            raise MudiffHipError(f'known_constrain: {name} must be {dt} of shape {tuple(known.shape)}, got {v.dtype} {tuple(v.shape)}')
    if mask is not None and x_new is None:
        raise MudiffHipError('known_constrain: x_new may be None only without a mask')
    known, noise, out = _contiguous_into('known_constrain', known, noise, out)
    x_new, mask = (None if v is None else v.contiguous() for v in (x_new, mask))
    t, a_tab, s_tab, kd = _level_and_keys('known_constrain', clean, t, a_tab, s_tab, noise, keys, rows, known.device)
    return known_constrain_into(out, x_new, known, mask, kd, _seed64(seed), step, kind, t, toff, a_tab, s_tab, clean, noise)


def known_coverage(M, src_shape, out_shape, device=None):
    """uint8 [Z, Y, X] on `device`: 1 where the voxel of the grid `out_shape` = (X, Y, Z) maps through M (volume_regrid.grid_matrix: 3 x 4
    or 4 x 4) to a source coordinate inside [0, S - 1] on all three axes of `src_shape` = (SX, SY, SZ): interpolated from acquired voxels
    alone (mud_known_coverage)."""
    m = np.ascontiguousarray(np.asarray(M, np.float64)[:3, :4])
    if m.shape != (3, 4):
        raise ValueError(f'known_coverage: need a 3 x 4 or 4 x 4 matrix, got {np.shape(M)}')
    SX, SY, SZ = (int(v) for v in src_shape)
    X, Y, Z = (int(v) for v in out_shape)
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.empty(max(Z, 0), max(Y, 0), max(X, 0), device=dev, dtype=torch.uint8)
    _launch('known_coverage', dev, load().mud_known_coverage, (C.c_double * 12)(*m.reshape(-1).tolist()), SX, SY, SZ, X, Y, Z, ptr(out), STREAM,
            nbytes=float(out.numel()))
    return out


# ---------------------------------------------------------------------------------------------------
# sampling a target acquired undersampled in k-space (csrc/kspace.hip, mudiff_hip.kspace)
KIND_KSPACE = 5                      # the draw of mud_kspace_constrain: the measured coefficients' forward noise
KSPACE_SIZES = (16, 32, 64, 128, 256, 512)


def kspace_size_ok(S):
    """S x S is a grid the k-space kernels take: a power of two in [16, 512]."""
    return int(S) in KSPACE_SIZES


def fft2(x, inverse=False, out=None):
    """The unitary 2D DFT of every slice of x [rows, S, S] (mud_fft2_c2c / mud_fft2_r2c): DC at [0, 0], scale 1/S; `inverse`: its adjoint.
    x: complex64, or real fp32 (the bits of the complex transform of (x, 0)).  out: None (a new complex64 tensor), a contiguous complex64
    tensor of the shape, or x itself for a complex x (in place).  S: a power of two in [16, 512]."""
    require_gpu(x, out)
    if x.dtype not in (torch.float32, torch.complex64) or x.dim() != 3 or x.shape[0] < 1 or x.shape[1] != x.shape[2]:
        raise MudiffHipError(f'fft2: x must be fp32 or complex64 [rows, S, S], got {x.dtype} {tuple(x.shape)}')
    rows, S = int(x.shape[0]), int(x.shape[1])
    if not kspace_size_ok(S):
        raise MudiffHipError(f'fft2: S must be a power of two in [16, 512], got {S}')
    real = x.dtype == torch.float32
    if out is not None and (out.dtype != torch.complex64 or out.shape != x.shape or not out.is_contiguous()):
        raise MudiffHipError(f'fft2: out must be a contiguous complex64 tensor of shape {tuple(x.shape)}, got {out.dtype} {tuple(out.shape)}')
    x = x if x.is_contiguous() else x.contiguous()
    out = torch.empty(x.shape, device=x.device, dtype=torch.complex64) if out is None else out
    fn = load().mud_fft2_r2c if real else load().mud_fft2_c2c
    _launch('fft2', x.device, fn, ptr(x), ptr(out), rows, S, int(bool(inverse)), STREAM, nbytes=float(x.numel() * (28 if real else 32)))
    return out


def _kspace_grid(name, x_new):
    """x_new: fp32 [rows, S, S] or [rows, 1, S, S] on a grid the transform takes -> (rows, S)."""
    if x_new.dtype != torch.float32 or x_new.dim() not in (3, 4) or x_new.shape[0] < 1 or x_new.shape[-1] != x_new.shape[-2] or \
            (x_new.dim() == 4 and x_new.shape[1] != 1):
        raise MudiffHipError(f'{name}: x_new must be fp32 [rows, S, S] or [rows, 1, S, S], got {x_new.dtype} {tuple(x_new.shape)}')
    if not kspace_size_ok(x_new.shape[-1]):
        raise MudiffHipError(f'{name}: S must be a power of two in [16, 512], got {int(x_new.shape[-1])}')
    return int(x_new.shape[0]), int(x_new.shape[-1])


def _kspace_operands(name, x_new, count, y, mask, noise, out, work):
    """What the two k-space wrappers share once _kspace_grid has passed x_new: y complex64 [count, S, S], mask uint8 [1 or count, S, S],
    _noise_and_out, and `work`, None or a contiguous complex64 [count, S, S] -> (x_new, y, mask, noise, out, work), contiguous, out and
    work allocated where they were not given.  count: the rows, or the groups of a slab measurement (its tables are built between the
    two checks, so a doubly bad call is refused as it always was)."""
    want = (count,) + tuple(x_new.shape[-2:])
    if y is None or y.dtype != torch.complex64 or tuple(y.shape) != want:
        raise MudiffHipError(f'{name}: y must be complex64 {want}, got {None if y is None else (y.dtype, tuple(y.shape))}')
    if mask is None or mask.dtype != torch.uint8 or mask.dim() != 3 or mask.shape[0] not in (1, count) or tuple(mask.shape[1:]) != want[1:]:
        raise MudiffHipError(f'{name}: mask must be uint8 [1 or {count}, {want[1]}, {want[2]}], got '
                             f'{None if mask is None else (mask.dtype, tuple(mask.shape))}')
    x_new, noise, out = _noise_and_out(name, x_new, noise, out)
    if work is not None and (work.dtype != torch.complex64 or tuple(work.shape) != want or not work.is_contiguous()):
        raise MudiffHipError(f'{name}: work must be a contiguous complex64 {want}, got {work.dtype} {tuple(work.shape)}')
    work = torch.empty(want, device=x_new.device, dtype=torch.complex64) if work is None else work
    return x_new, y.contiguous(), mask.contiguous(), noise, out, work


def kspace_constrain_into(out, x_new, y, mask, work, keys_dev, seed, step, kind, t, toff, a_tab, s_tab, clean=False, noise=None):
    """Unchecked launch of mud_kspace_constrain into `out` (fp32, contiguous, [rows, ..., S, S]; may be x_new): GraphSampler.sample_keyed
    checks its operands once per batch, not once per step.  y, work: complex64 [rows, S, S]; mask: uint8 [1 or rows, S, S]; keys_dev:
    through check_keys and on out's device (None with `noise` or `clean`)."""
    rows, S = out.shape[0], out.shape[-1]
    _launch('kspace_constrain', out.device, load().mud_kspace_constrain, ptr(x_new), ptr(y), ptr(mask), int(mask.shape[0]),
            *_level_args(noise, keys_dev, seed, step, kind, t, toff, a_tab, s_tab, clean), ptr(out), ptr(work), rows, S, STREAM,
            nbytes=float(out.numel() * 44))
    return out


def kspace_constrain(x_new, y, mask, t, toff, a_tab, s_tab, *, noise=None, keys=None, seed=0, step=0, kind=KIND_KSPACE, clean=False, out=None,
                     work=None):
    """out = x_new - Re F^H[ mask ? F(x_new - s_tab[c] * eta) - a_tab[c] * y : 0 ] per slice, c = clamp(t[row] + toff, 0, len(a_tab) - 1);
    with `clean`, out = x_new - Re F^H[ mask ? F(x_new) - y : 0 ] (mud_kspace_constrain; F: ops.fft2).  F is unitary, so the measured
    coefficients of x_new become those of q_sample(k, c) for y = mask * F(k) and the others stay.  x_new: fp32 [rows, S, S] or
    [rows, 1, S, S]; y: complex64 [rows, S, S]; mask: uint8 [1 or rows, S, S], non-zero = measured (pass a Hermitian-symmetric one, or the
    real part taken at the end halves the unpaired coefficients' correction).  eta: `noise` (fp32, x_new's shape) when given, else the keyed normal
    ops.randn_keyed gives keys[r] = (slice, sample) under (seed, step, kind), drawn in the kernel.  t: int64 [rows]; with `clean` it, the
    tables and the draw are not needed.  out: None (a new tensor), x_new (in place) or a contiguous fp32 tensor of the shape.  work: None
    or a contiguous complex64 [rows, S, S] workspace (overwritten)."""
    require_gpu(x_new, y, mask, noise, t, a_tab, s_tab, out, work)
    rows, _ = _kspace_grid('kspace_constrain', x_new)
    x_new, y, mask, noise, out, work = _kspace_operands('kspace_constrain', x_new, rows, y, mask, noise, out, work)
    t, a_tab, s_tab, kd = _level_and_keys('kspace_constrain', clean, t, a_tab, s_tab, noise, keys, rows, x_new.device)
    return kspace_constrain_into(out, x_new, y, mask, work, kd, _seed64(seed), step, kind, t, toff, a_tab, s_tab, clean, noise)


# ---------------------------------------------------------------------------------------------------
# sampling a target acquired with thick slices (csrc/slab.hip, mudiff_hip.thick)
KIND_THICK = 6                       # the draw of mud_slab_constrain: the slab averages' forward noise
SLAB_MAX_MEMBERS = 16                # include/mudiff_hip.h: MUD_SLAB_MAX_MEMBERS


def slab_gains(weights):
    """g_l = w_l / sum_m w_m^2 per group (an unused slot's weight counts as it stands: pass 0 there), in fp64, rounded once to fp32."""
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    w = w.reshape(1, -1) if w.ndim == 1 else w
    return (w / (w * w).sum(1, keepdims=True)).astype(np.float32)


def slab_tables(members, weights, gains=None):
    """The host tables of mud_slab_constrain / mud_slab_average, read at call time: (members int32 [groups, L], weights fp32 [groups, L],
    gains fp32 [groups, L]) as contiguous numpy arrays.  members: row indices, -1 = an unused tail; weights [L] serves every group;
    gains None: slab_gains of the weights with the unused slots' weights taken as 0.  Only shapes are checked here: the entry refuses a
    bad index, a row named twice, an empty group and a bad weight before it launches anything."""
    m = np.ascontiguousarray(np.asarray(members, dtype=np.int32))
    m = m.reshape(1, -1) if m.ndim == 1 else m
    if m.ndim != 2 or m.shape[1] < 1:
        raise MudiffHipError(f'slab_tables: members must be [groups, L] with L >= 1, got {m.shape}')
    w = np.asarray(weights, dtype=np.float32)
    w = np.ascontiguousarray(np.broadcast_to(w, m.shape)) if w.ndim == 1 and w.shape[0] == m.shape[1] else np.ascontiguousarray(w)
    if w.shape != m.shape:
        raise MudiffHipError(f'slab_tables: weights must be [L] or {m.shape}, got {w.shape}')
    g = slab_gains(np.where(m >= 0, w, np.float32(0))) if gains is None else np.ascontiguousarray(np.asarray(gains, dtype=np.float32))
    g = np.ascontiguousarray(np.broadcast_to(g, m.shape)) if g.ndim == 1 and g.shape[0] == m.shape[1] else g
    if g.shape != m.shape:
        raise MudiffHipError(f'slab_tables: gains must be [L] or {m.shape}, got {g.shape}')
    return m, w, g


def _host(a):
    return C.c_void_p(a.ctypes.data)


def slab_constrain_into(out, x_new, y, tables, keys_dev, seed, step, kind, t, toff, a_tab, s_tab, clean=False, noise=None):
    """Unchecked launch of mud_slab_constrain into `out` (fp32, contiguous, [rows, ...]; may be x_new): GraphSampler.sample_keyed checks
    its operands once per batch, not once per step.  y: fp32 [groups, row_len]; tables: slab_tables'; keys_dev: through check_keys and on
    out's device (None with `noise` or `clean`)."""
    rows = out.shape[0]
    m, w, g = tables
    groups, L = m.shape
    row_len = out.numel() // max(rows, 1)
    _launch('slab_constrain', out.device, load().mud_slab_constrain, ptr(x_new), ptr(y), _host(m), _host(w), _host(g), groups, L,
            *_level_args(noise, keys_dev, seed, step, kind, t, toff, a_tab, s_tab, clean), ptr(out), rows, row_len, STREAM,
            nbytes=float(row_len * 4 * (3 * int((m >= 0).sum()) + groups)))
    return out


def slab_constrain(x_new, y, members, weights, t, toff, a_tab, s_tab, *, gains=None, noise=None, keys=None, seed=0, step=0, kind=KIND_THICK,
                   clean=False, out=None):
    """The data-consistency step of thick-slice measurements (mud_slab_constrain).  Group j names the rows members[j] (its thin slices,
    -1 = unused) with weights w and gains g (slab_tables); with c = clamp(t[first member] + toff, 0, len(a_tab) - 1), per element
        r = sum_l w_l (x_new[m_l] - s_tab[c] * eta[m_l]) - a_tab[c] * y[j]        (clean: r = sum_l w_l x_new[m_l] - y[j])
        out[m_l] = x_new[m_l] - g_l * r,
    summed in the table's order, so that the slab average of the result is that of q_sample(k, c) for y = sum_l w_l k_l and everything
    orthogonal to the profile is untouched.  A row of no group is copied bit for bit.  x_new: fp32 [rows, ...]; y: fp32 [groups, ...] with
    x_new's row shape.  eta: `noise` (fp32, x_new's shape) when given, else the keyed normal ops.randn_keyed gives keys[r] = (slice, sample)
    under (seed, step, kind), drawn in the kernel.  t: int64 [rows]; with `clean` it, the tables and the draw are not needed.  out: None (a
    new tensor), x_new (in place) or a contiguous fp32 tensor of the shape."""
    require_gpu(x_new, y, noise, t, a_tab, s_tab, out)
    if x_new.dtype != torch.float32 or x_new.dim() < 1 or x_new.shape[0] < 1 or x_new[0].numel() < 1:
        raise MudiffHipError(f'slab_constrain: x_new must be a non-empty fp32 [rows, ...] tensor, got {x_new.dtype} {tuple(x_new.shape)}')
    rows = x_new.shape[0]
    tables = slab_tables(members, weights, gains)
    groups = tables[0].shape[0]
    if y is None or y.dtype != torch.float32 or y.dim() < 1 or y.shape[0] != groups or y.numel() != groups * x_new[0].numel():
        raise MudiffHipError(f'slab_constrain: y must be fp32 [{groups}, {x_new[0].numel()}], got '
                             f'{None if y is None else (y.dtype, tuple(y.shape))}')
    x_new, noise, out = _noise_and_out('slab_constrain', x_new, noise, out)
    t, a_tab, s_tab, kd = _level_and_keys('slab_constrain', clean, t, a_tab, s_tab, noise, keys, rows, x_new.device)
    return slab_constrain_into(out, x_new, y.contiguous(), tables, kd, _seed64(seed), step, kind, t, toff, a_tab, s_tab, clean, noise)


def slab_average(x, members, weights, out=None):
    """avg[j] = sum_l w_l x[members[j][l]] per element, in mud_slab_constrain's order and rounding (mud_slab_average): the measurement y of
    k, and A x of the residual.  x: fp32 [rows, ...] -> fp32 [groups, ...]."""
    require_gpu(x, out)
    if x.dtype != torch.float32 or x.dim() < 1 or x.shape[0] < 1 or x[0].numel() < 1:
        raise MudiffHipError(f'slab_average: x must be a non-empty fp32 [rows, ...] tensor, got {x.dtype} {tuple(x.shape)}')
    m, w, _ = slab_tables(members, weights, weights)
    groups, L = m.shape
    shape = (groups,) + tuple(x.shape[1:])
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous()):
        raise MudiffHipError(f'slab_average: out must be a contiguous fp32 tensor of shape {shape}, got {out.dtype} {tuple(out.shape)}')
    x = x if x.is_contiguous() else x.contiguous()
    out = torch.empty(shape, device=x.device, dtype=torch.float32) if out is None else out
    row_len = x[0].numel()
    _launch('slab_average', x.device, load().mud_slab_average, ptr(x), _host(m), _host(w), groups, L, ptr(out), int(x.shape[0]), row_len, STREAM,
            nbytes=float(row_len * 4 * (int((m >= 0).sum()) + groups)))
    return out


# ---------------------------------------------------------------------------------------------------
# sampling a target acquired as accelerated thick slices (csrc/slab_kspace.hip, mudiff_hip.multislice)
KIND_MULTISLICE = 7                  # the draw of mud_slab_kspace_constrain: the slab averages' measured coefficients' forward noise


def slab_kspace_constrain_into(out, x_new, y, mask, tables, work, keys_dev, seed, step, kind, t, toff, a_tab, s_tab, clean=False, noise=None):
    """Unchecked launch of mud_slab_kspace_constrain into `out` (fp32, contiguous, [rows, ..., S, S]; may be x_new): GraphSampler.
    sample_keyed checks its operands once per batch, not once per step.  y, work: complex64 [groups, S, S]; mask: uint8 [1 or groups, S, S];
    tables: slab_tables'; keys_dev: through check_keys and on out's device (None with `noise` or `clean`)."""
    rows, S = out.shape[0], out.shape[-1]
    m, w, g = tables
    groups, L = m.shape
    _launch('slab_kspace_constrain', out.device, load().mud_slab_kspace_constrain, ptr(x_new), ptr(y), ptr(mask), int(mask.shape[0]), _host(m), _host(w),
            _host(g), groups, L, *_level_args(noise, keys_dev, seed, step, kind, t, toff, a_tab, s_tab, clean), ptr(out), ptr(work), rows, S, STREAM,
            nbytes=float(S * S * (12 * int((m >= 0).sum()) + 41 * groups)))
    return out


def slab_kspace_constrain(x_new, y, mask, members, weights, t, toff, a_tab, s_tab, *, gains=None, noise=None, keys=None, seed=0, step=0,
                          kind=KIND_MULTISLICE, clean=False, out=None, work=None):
    """The data-consistency step of accelerated thick-slice measurements (mud_slab_kspace_constrain).  Group j names the rows members[j]
    (its thin slices, -1 = unused) with weights w and gains g (slab_tables); with c = clamp(t[first member] + toff, 0, len(a_tab) - 1)
        d = sum_l w_l (x_new[m_l] - s_tab[c] * eta[m_l])                         (clean: d = sum_l w_l x_new[m_l])
        out[m_l] = x_new[m_l] - g_l * Re F^H[ mask ? F(d) - a_tab[c] * y[j] : 0 ]     (clean: ... - y[j]),
    summed in the table's order (F: ops.fft2), so that the measured coefficients of the slab average of the result are those of
    q_sample(k, c) for y = mask * F(sum_l w_l k_l); the other coefficients and everything orthogonal to the profile are untouched.  A row
    of no group is copied bit for bit.  x_new: fp32 [rows, S, S] or [rows, 1, S, S]; y: complex64 [groups, S, S]; mask: uint8
    [1 or groups, S, S], non-zero = measured (pass a Hermitian-symmetric one).  eta: `noise` (fp32, x_new's shape) when given, else the keyed
    normal ops.randn_keyed gives keys[r] = (slice, sample) under (seed, step, kind), drawn in the kernel.  t: int64 [rows]; with `clean`
    it, the tables and the draw are not needed.  out: None (a new tensor), x_new (in place) or a contiguous fp32 tensor of the shape.
    work: None or a contiguous complex64 [groups, S, S] workspace (overwritten)."""
    require_gpu(x_new, y, mask, noise, t, a_tab, s_tab, out, work)
    rows, _ = _kspace_grid('slab_kspace_constrain', x_new)
    tables = slab_tables(members, weights, gains)
    x_new, y, mask, noise, out, work = _kspace_operands('slab_kspace_constrain', x_new, tables[0].shape[0], y, mask, noise, out, work)
    t, a_tab, s_tab, kd = _level_and_keys('slab_kspace_constrain', clean, t, a_tab, s_tab, noise, keys, rows, x_new.device)
    return slab_kspace_constrain_into(out, x_new, y, mask, tables, work, kd, _seed64(seed), step, kind, t, toff, a_tab, s_tab, clean, noise)


# ---------------------------------------------------------------------------------------------------
# sampling a target given as a thick-slice volume of its own geometry (csrc/band.hip, mudiff_hip.thick_volume)
KIND_BAND = 8                        # the draw of mud_band_constrain: the thick slices' forward noise
BAND_MAX_MEMBERS, BAND_MAX_BW, BAND_MAX_M, BAND_MAX_N = 32, 8, 256, 512      # include/mudiff_hip.h: MUD_BAND_MAX_*
BAND_MAX_COND = 1e4                  # cond(A A^T) <= 1e4: 1e4 * 2^-24 ~ 6e-4 keeps the fp32 solve inside the 1e-3 parity bar


class BandTables:
    """The tables of mud_band_constrain / mud_band_measure for a measurement matrix A [m, n] (band_tables): numpy arrays `start`,
    `member`, `w` (the CSR of A by thick slice), `tstart`, `tmember`, `tw` (of A^T by thin slice), `lc` [m, bw + 1] (the banded Cholesky
    factor of G = A A^T, lc[j, 0] = 1 / L[j, j], lc[j, k] = L[j, j - k]), and m, n, bw, nnz, cond (of G, fp64).  `A32` is A as the kernel
    sees it, the fp32 weights in fp64.  `on(device)` uploads them once per device -> the struct the entries take."""

    def __init__(self, m, n, bw, start, member, w, tstart, tmember, tw, lc, cond, A32):
        self.m, self.n, self.bw, self.nnz, self.cond, self.A32 = int(m), int(n), int(bw), int(member.shape[0]), float(cond), A32
        self.start, self.member, self.w, self.tstart, self.tmember, self.tw, self.lc = start, member, w, tstart, tmember, tw, lc
        self._dev = {}

    def on(self, device):
        device = torch.device(device)
        key = (device.type, torch.cuda.current_device() if device.index is None else device.index)
        if key not in self._dev:
            from . import BandTables as Struct
            t = [torch.from_numpy(a).to(device) for a in (self.start, self.member, self.w, self.tstart, self.tmember, self.tw, self.lc.reshape(-1))]
            self._dev[key] = (Struct(self.m, self.n, self.bw, self.nnz, *(v.data_ptr() for v in t)), t)      # t: keeps the memory alive
        return self._dev[key][0]


def band_tables(A):
    """A: the measurement matrix of thick slices, dense fp64 [m, n] or CSR as (start [m + 1], member [nnz], w [nnz], n) -> BandTables.
    Row j's non-zeros become its members in thin-slice order; the weights are rounded once to fp32, and G = A A^T, its bandwidth, its
    fp64 eigenvalues and its Cholesky factor are those of the rounded weights.  ValueError for m > 256, n > 512, a row with no member or
    more than 32, a bandwidth above 8, a weight that is not finite, and for cond(G) > 1e4 (or a G that is not positive definite: two
    coincident thick slices)."""
    if isinstance(A, (tuple, list)) and len(A) == 4:
        st, mem, ww, n = A
        st, mem, ww = np.asarray(st, np.int64), np.asarray(mem, np.int64), np.asarray(ww, np.float64)
        if st.ndim != 1 or st.shape[0] < 2 or st[0] != 0 or st[-1] != mem.shape[0] or mem.shape != ww.shape or np.any(np.diff(st) < 0):
            raise ValueError('band_tables: CSR must be (start [m + 1] from 0 to nnz, member [nnz], w [nnz], n)')
        if mem.size and (mem.min() < 0 or mem.max() >= int(n)):
            raise ValueError(f'band_tables: a member lies outside [0, {int(n)})')
        dense = np.zeros((st.shape[0] - 1, int(n)), np.float64)
        for j in range(st.shape[0] - 1):
            np.add.at(dense[j], mem[st[j]:st[j + 1]], ww[st[j]:st[j + 1]])
        A = dense
    A = np.asarray(A, np.float64)
    if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] < 1:
        raise ValueError(f'band_tables: A must be [m, n], got {A.shape}')
    m, n = A.shape
    if m > BAND_MAX_M or n > BAND_MAX_N:
        raise ValueError(f'band_tables: at most {BAND_MAX_M} thick and {BAND_MAX_N} thin slices, got {m} and {n}')
    if not np.all(np.isfinite(A)):
        raise ValueError('band_tables: A holds a weight that is not finite')
    A32 = A.astype(np.float32).astype(np.float64)
    counts = (A32 != 0).sum(1)
    if counts.min() < 1 or counts.max() > BAND_MAX_MEMBERS:
        raise ValueError(f'band_tables: a thick slice must have 1 to {BAND_MAX_MEMBERS} members, got {int(counts.min())} to {int(counts.max())}')
    G = A32 @ A32.T
    jj, kk = np.nonzero(G)
    bw = int(np.abs(jj - kk).max())
    if bw > BAND_MAX_BW:
        raise ValueError(f'band_tables: A A^T has bandwidth {bw}, at most {BAND_MAX_BW} is supported')
    ev = np.linalg.eigvalsh(G)
    cond = float(ev[-1] / ev[0]) if ev[0] > 0 else math.inf
    if not cond <= BAND_MAX_COND:
        raise ValueError(f'band_tables: cond(A A^T) = {cond:.3g} exceeds {BAND_MAX_COND:g}: the thick slices are (nearly) dependent and the '
                         'fp32 solve would leave the 1e-3 parity bar')
    L = np.linalg.cholesky(G)
    lc = np.zeros((m, bw + 1), np.float64)
    lc[:, 0] = 1.0 / np.diag(L)
    for k in range(1, bw + 1):
        lc[k:, k] = np.diag(L, -k)
    start = np.zeros(m + 1, np.int32)
    start[1:] = np.cumsum(counts)
    rows, cols = np.nonzero(A32)                             # row-major: thin index ascending within a thick slice
    tcols, trows = np.nonzero(A32.T)                         # thick index ascending within a thin slice
    tstart = np.zeros(n + 1, np.int32)
    tstart[1:] = np.cumsum((A32 != 0).sum(0))
    c = np.ascontiguousarray
    return BandTables(m, n, bw, start, c(cols.astype(np.int32)), c(A32[rows, cols].astype(np.float32)), tstart, c(trows.astype(np.int32)),
                      c(A32[trows, tcols].astype(np.float32)), c(lc.astype(np.float32)), cond, A32)


def band_constrain_into(out, x, y, tables, work, keys_dev, seed, step, kind, t, toff, a_tab, s_tab, clean=False, noise=None):
    """Unchecked launch of mud_band_constrain into `out` (fp32, contiguous, sets * n rows; may be x): GraphSampler.sample_lockstep checks
    its operands once, not once per step.  y: fp32 [m, row_len]; tables: band_tables'; work: fp32, sets * m rows; keys_dev: through
    check_keys and on out's device (None with `noise` or `clean`)."""
    row_len = y.numel() // tables.m
    sets = out.numel() // (tables.n * row_len)
    _launch('band_constrain', out.device, load().mud_band_constrain, ptr(x), ptr(y), C.byref(tables.on(out.device)),
            *_level_args(noise, keys_dev, seed, step, kind, t, toff, a_tab, s_tab, clean), ptr(out), ptr(work), sets, row_len, STREAM,
            nbytes=float(row_len * 4 * (sets * (2 * tables.nnz + 2 * tables.n + 4 * tables.m) + tables.m)))
    return out


def _band_shapes(name, x, tables):
    """x: fp32 [sets, n, ...] -> (sets, row_len)."""
    if not isinstance(tables, BandTables):
        raise MudiffHipError(f'{name}: tables must come from ops.band_tables')
    if x.dtype != torch.float32 or x.dim() < 3 or x.numel() < 1 or x.shape[1] != tables.n:
        raise MudiffHipError(f'{name}: x must be a non-empty fp32 [sets, {tables.n}, ...] tensor, got {x.dtype} {tuple(x.shape)}')
    sets, row_len = int(x.shape[0]), x[0, 0].numel()
    if sets * max(tables.n, tables.m) * row_len >= 1 << 31 or sets > 65535:
        raise MudiffHipError(f'{name}: sets * max(m, n) * row_len must be < 2^31 and sets <= 65535, got {sets} x {max(tables.n, tables.m)} x {row_len}')
    return sets, row_len


def band_constrain(x, y, tables, t, toff, a_tab, s_tab, *, noise=None, keys=None, seed=0, step=0, kind=KIND_BAND, clean=False, out=None,
                   work=None):
    """The data-consistency step of thick slices with a geometry of their own (mud_band_constrain).  With A = tables.A32 [m, n],
    G = A A^T and c = clamp(t[first row of the set] + toff, 0, len(a_tab) - 1), per element of every set
        out = x - A^T G^-1 (A (x - s_tab[c] * eta) - a_tab[c] * y)                  (clean: out = x - A^T G^-1 (A x - y)),
    the solve by the banded Cholesky factor of the tables, so that A out is A q_sample(k, c) for y = A k and everything orthogonal to
    the rows of A is untouched.  A thin slice under no thick slice is copied bit for bit.  x: fp32 [sets, n, ...] (a set: one sample's
    whole stack); y: fp32 [m, ...] with x's row shape, shared by the sets.  eta: `noise` (fp32, x's shape) when given, else the keyed normal
    ops.randn_keyed gives keys[r] = (slice, sample) of row r = set * n + i under (seed, step, kind), drawn in the kernel.  t: int64
    [sets * n]; with `clean` it, the tables and the draw are not needed.  out: None (a new tensor), x (in place) or a contiguous fp32
    tensor of the shape.  work: None or a contiguous fp32 workspace of sets * m rows (overwritten)."""
    require_gpu(x, y, noise, t, a_tab, s_tab, out, work)
    sets, row_len = _band_shapes('band_constrain', x, tables)
    rows = sets * tables.n
    if y is None or y.dtype != torch.float32 or y.dim() < 1 or y.shape[0] != tables.m or y.numel() != tables.m * row_len:
        raise MudiffHipError(f'band_constrain: y must be fp32 [{tables.m}, {row_len}], got {None if y is None else (y.dtype, tuple(y.shape))}')
    x, noise, out = _noise_and_out('band_constrain', x, noise, out)
    if work is not None and (work.dtype != torch.float32 or work.numel() != sets * tables.m * row_len or not work.is_contiguous()):
        raise MudiffHipError(f'band_constrain: work must be a contiguous fp32 tensor of {sets * tables.m} x {row_len} elements')
    t, a_tab, s_tab, kd = _level_and_keys('band_constrain', clean, t, a_tab, s_tab, noise, keys, rows, x.device)
    work = torch.empty(sets * tables.m, row_len, device=x.device, dtype=torch.float32) if work is None else work
    return band_constrain_into(out, x, y.contiguous(), tables, work, kd, _seed64(seed), step, kind, t, toff, a_tab, s_tab, clean, noise)


def band_measure(x, tables, out=None):
    """ax[set, j] = sum_s w_js x[set, member_js] per element, in mud_band_constrain's order and rounding (mud_band_measure): the
    measurement y of k, and A x of the residual.  x: fp32 [sets, n, ...] -> fp32 [sets, m, ...]."""
    require_gpu(x, out)
    sets, row_len = _band_shapes('band_measure', x, tables)
    shape = (sets, tables.m) + tuple(x.shape[2:])
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous()):
        raise MudiffHipError(f'band_measure: out must be a contiguous fp32 tensor of shape {shape}, got {out.dtype} {tuple(out.shape)}')
    x = x if x.is_contiguous() else x.contiguous()
    out = torch.empty(shape, device=x.device, dtype=torch.float32) if out is None else out
    _launch('band_measure', x.device, load().mud_band_measure, ptr(x), C.byref(tables.on(x.device)), ptr(out), sets, row_len, STREAM,
            nbytes=float(row_len * 4 * sets * (tables.nnz + tables.m)))
    return out


# ---------------------------------------------------------------------------------------------------
# sampling a target given as a volume coarser than the stack in all three axes (csrc/lowres.hip, mudiff_hip.lowres_volume; DESIGN.md
# section 5.31)
KIND_LOWRES = 9                      # the draw of mud_lowres_constrain: the coarse voxels' forward noise


class LowresTables:
    """The three BandTables of mud_lowres_constrain / mud_lowres_measure (lowres_tables): `z` over the thin slices, `y` over the image
    rows, `x` over the image columns, and `cond` = cond(G_z) cond(G_y) cond(G_x), the condition number of A A^T for A = A_z (x) A_y (x) A_x."""

    def __init__(self, z, y, x):
        self.z, self.y, self.x = z, y, x
        self.cond = z.cond * y.cond * x.cond
        self.shape = (z.m, y.m, x.m)

    def on(self, device):
        return tuple(C.byref(t.on(device)) for t in (self.z, self.y, self.x))


def lowres_tables(A_z, A_y, A_x):
    """A_z [m_z, n], A_y [m_y, H], A_x [m_x, W] (each as band_tables takes it) -> LowresTables.  Every axis keeps band_tables' own limits;
    ValueError in addition when cond(G_z) cond(G_y) cond(G_x) > 1e4: the Kronecker product's condition number is the product, and the
    fp32 solves run one after the other."""
    tabs = LowresTables(band_tables(A_z), band_tables(A_y), band_tables(A_x))
    if not tabs.cond <= BAND_MAX_COND:
        raise ValueError(f'lowres_tables: cond(A A^T) = {tabs.z.cond:.3g} x {tabs.y.cond:.3g} x {tabs.x.cond:.3g} = {tabs.cond:.3g} exceeds '
                         f'{BAND_MAX_COND:g}: the coarse voxels are (nearly) dependent and the fp32 solve would leave the 1e-3 parity bar')
    return tabs


def lowres_ws_floats(sets, tables):
    """The floats of the workspace of lowres_constrain / lowres_measure for `sets` sets (mud_lowres_ws_floats)."""
    return int(load().mud_lowres_ws_floats(int(sets), tables.z.n, *tables.shape))


def lowres_constrain_into(out, x, y, tables, work, keys_dev, seed, step, kind, t, toff, a_tab, s_tab, clean=False, noise=None):
    """Unchecked launch of mud_lowres_constrain into `out` (fp32, contiguous, [sets * n, H, W]; may be x): GraphSampler.sample_lockstep
    checks its operands once, not once per step.  y: fp32 [m_z, m_y, m_x]; tables: lowres_tables'; work: fp32, lowres_ws_floats
    elements; keys_dev: through check_keys and on out's device (None with `noise` or `clean`)."""
    H, W = tables.y.n, tables.x.n
    rows = out.numel() // (H * W)
    mz, my, mx = tables.shape
    _launch('lowres_constrain', out.device, load().mud_lowres_constrain, ptr(x), ptr(y), *tables.on(out.device), H, W, rows, ptr(work),
            *_level_args(noise, keys_dev, seed, step, kind, t, toff, a_tab, s_tab, clean), ptr(out), STREAM,
            nbytes=float(4 * (rows * (tables.y.nnz * W + 2 * H * W + my * mx * (1 + tables.z.nnz / tables.z.n)) + 8 * (rows // tables.z.n) * mz * my * mx)))
    return out


def _lowres_shapes(name, x, tables):
    """x: fp32 [sets, n, H, W] -> sets."""
    if not isinstance(tables, LowresTables):
        raise MudiffHipError(f'{name}: tables must come from ops.lowres_tables')
    want = (tables.z.n, tables.y.n, tables.x.n)
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[0] < 1 or tuple(x.shape[1:]) != want:
        raise MudiffHipError(f'{name}: x must be a non-empty fp32 [sets, {want[0]}, {want[1]}, {want[2]}] tensor, got {x.dtype} {tuple(x.shape)}')
    sets = int(x.shape[0])
    if x.numel() >= 1 << 31 or sets * want[0] > 65535:
        raise MudiffHipError(f'{name}: sets * n * H * W must be < 2^31 and sets * n <= 65535, got {tuple(x.shape)}')
    return sets


def lowres_constrain(x, y, tables, t, toff, a_tab, s_tab, *, noise=None, keys=None, seed=0, step=0, kind=KIND_LOWRES, clean=False, out=None,
                     work=None):
    """The data-consistency step of a target measured on a coarser grid in all three axes (mud_lowres_constrain).  With A = A_z (x) A_y
    (x) A_x of tables' three axes and c = clamp(t[first row of the set] + toff, 0, len(a_tab) - 1), per set
        out = x - A^T (A A^T)^-1 (A (x - s_tab[c] * eta) - a_tab[c] * y)             (clean: out = x - A^T (A A^T)^-1 (A x - y)),
    one banded Cholesky solve per axis, so that A out is A q_sample(k, c) for y = A k and everything orthogonal to the rows of A is
    untouched.  A pixel under no coarse voxel is copied bit for bit.  x: fp32 [sets, n, H, W] (a set: one sample's whole stack); y: fp32
    [m_z, m_y, m_x], shared by the sets.  eta: `noise` (fp32, x's shape) when given, else the keyed normal ops.randn_keyed gives
    keys[r] = (slice, sample) of row r = set * n + i under (seed, step, kind), drawn in the kernel.  t: int64 [sets * n]; with `clean`
    it, the level tables and the draw are not needed.  out: None (a new tensor), x (in place) or a contiguous fp32 tensor of the shape.
    work: None or a contiguous fp32 workspace of lowres_ws_floats(sets, tables) elements (overwritten)."""
    require_gpu(x, y, noise, t, a_tab, s_tab, out, work)
    sets = _lowres_shapes('lowres_constrain', x, tables)
    rows = sets * tables.z.n
    if y is None or y.dtype != torch.float32 or tuple(y.shape) != tables.shape:
        raise MudiffHipError(f'lowres_constrain: y must be fp32 {list(tables.shape)}, got {None if y is None else (y.dtype, tuple(y.shape))}')
    x, noise, out = _noise_and_out('lowres_constrain', x, noise, out)
    need = lowres_ws_floats(sets, tables)
    if work is not None and (work.dtype != torch.float32 or work.numel() != need or not work.is_contiguous()):
        raise MudiffHipError(f'lowres_constrain: work must be a contiguous fp32 tensor of {need} elements')
    t, a_tab, s_tab, kd = _level_and_keys('lowres_constrain', clean, t, a_tab, s_tab, noise, keys, rows, x.device)
    work = torch.empty(need, device=x.device, dtype=torch.float32) if work is None else work
    return lowres_constrain_into(out, x, y.contiguous(), tables, work, kd, _seed64(seed), step, kind, t, toff, a_tab, s_tab, clean, noise)


def lowres_measure(x, tables, out=None, work=None):
    """ax[set] = A x[set] on the coarse lattice, in mud_lowres_constrain's order and rounding (mud_lowres_measure): the measurement y
    of k, and A x of the residual.  x: fp32 [sets, n, H, W] -> fp32 [sets, m_z, m_y, m_x].  work: None or a contiguous fp32 workspace of
    at least sets * n * m_y * m_x elements (overwritten)."""
    require_gpu(x, out, work)
    sets = _lowres_shapes('lowres_measure', x, tables)
    shape = (sets,) + tables.shape
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous()):
        raise MudiffHipError(f'lowres_measure: out must be a contiguous fp32 tensor of shape {shape}, got {out.dtype} {tuple(out.shape)}')
    need = sets * tables.z.n * tables.y.m * tables.x.m
    if work is not None and (work.dtype != torch.float32 or work.numel() < need or not work.is_contiguous()):
        raise MudiffHipError(f'lowres_measure: work must be a contiguous fp32 tensor of at least {need} elements')
    x = x if x.is_contiguous() else x.contiguous()
    out = torch.empty(shape, device=x.device, dtype=torch.float32) if out is None else out
    work = torch.empty(need, device=x.device, dtype=torch.float32) if work is None else work
    _launch('lowres_measure', x.device, load().mud_lowres_measure, ptr(x), *tables.on(x.device), tables.y.n, tables.x.n, sets * tables.z.n, ptr(work),
            ptr(out), STREAM, nbytes=float(4 * sets * tables.z.n * (tables.y.nnz * tables.x.n + 2 * tables.y.m * tables.x.m)))
    return out


# ---------------------------------------------------------------------------------------------------
# sampling a target acquired accelerated on several coils (csrc/sense.hip, mudiff_hip.sense)
KIND_SENSE = 10                      # the draw of mud_sense_constrain: the measurement's forward noise, in the image domain
KIND_SENSE_MEAS = 11                 # the measurement noise of mudiff_hip.sense (--sense_noise): key (slice, coil), row length 2 S^2
SENSE_MAX_COILS, SENSE_MAX_ITERS = 32, 64      # include/mudiff_hip.h: MUD_SENSE_MAX_COILS, the largest `iters`


def sense_ws_floats(rows, coils, S):
    """The floats of the workspace of sense_constrain for a batch of `rows` slices (mud_sense_ws_floats)."""
    n = int(load().mud_sense_ws_floats(int(rows), int(coils), int(S)))
    if n < 0:
        raise MudiffHipError(f'sense_ws_floats: rows >= 1, coils in [1, {SENSE_MAX_COILS}] and S a power of two in [16, 512], got {rows}, {coils}, {S}')
    return n


def _sense_maps(name, maps, rows, S, mask=None):
    """maps: complex64 [coils, S, S] (one set for every row) or [rows, coils, S, S]; mask: None or uint8 [1 or rows, S, S] -> (maps as
    [map_rows, coils, S, S], mask), contiguous."""
    if maps is None or maps.dtype != torch.complex64 or maps.dim() not in (3, 4) or tuple(maps.shape[-2:]) != (S, S) or \
            (maps.dim() == 4 and maps.shape[0] not in (1, rows)) or not 1 <= maps.shape[-3] <= SENSE_MAX_COILS:
        raise MudiffHipError(f'{name}: maps must be complex64 [coils, {S}, {S}] or [1 or {rows}, coils, {S}, {S}] with coils in [1, {SENSE_MAX_COILS}], '
                             f'got {None if maps is None else (maps.dtype, tuple(maps.shape))}')
    maps = (maps[None] if maps.dim() == 3 else maps).contiguous()
    if maps.numel() // maps.shape[0] * rows >= 1 << 31:
        raise MudiffHipError(f'{name}: rows * coils * S * S must be < 2^31, got {rows} x {tuple(maps.shape[1:])}')
    if mask is not None and (mask.dtype != torch.uint8 or mask.dim() != 3 or mask.shape[0] not in (1, rows) or tuple(mask.shape[1:]) != (S, S)):
        raise MudiffHipError(f'{name}: mask must be uint8 [1 or {rows}, {S}, {S}], got {mask.dtype} {tuple(mask.shape)}')
    return maps, None if mask is None else mask.contiguous()


def sense_measure(x, maps, mask, out=None):
    """y = mask .* F(C_c x) per coil (mud_sense_measure; F: ops.fft2): x fp32 [rows, S, S], maps complex64 [coils, S, S] or [1 or rows,
    coils, S, S], mask uint8 [1 or rows, S, S] (non-zero = measured; not symmetrised: C_c x is complex) -> complex64 [rows, coils, S, S]."""
    require_gpu(x, maps, mask, out)
    if x.dim() != 3:
        raise MudiffHipError(f'sense_measure: x must be fp32 [rows, S, S], got {x.dtype} {tuple(x.shape)}')
    rows, S = _kspace_grid('sense_measure', x)
    if mask is None:
        raise MudiffHipError('sense_measure: mask is needed')
    maps, mask = _sense_maps('sense_measure', maps, rows, S, mask)
    shape = (rows, maps.shape[1], S, S)
    if out is not None and (out.dtype != torch.complex64 or tuple(out.shape) != shape or not out.is_contiguous()):
        raise MudiffHipError(f'sense_measure: out must be a contiguous complex64 tensor of shape {shape}, got {out.dtype} {tuple(out.shape)}')
    out = torch.empty(shape, device=x.device, dtype=torch.complex64) if out is None else out
    _launch('sense_measure', x.device, load().mud_sense_measure, ptr(x.contiguous()), ptr(maps), int(maps.shape[0]), int(maps.shape[1]), ptr(mask),
            int(mask.shape[0]), ptr(out), rows, S, STREAM, nbytes=float(out.numel() * 32))
    return out


def sense_adjoint(y, maps, out=None):
    """Re sum_c conj(C_c) F^H y_c (mud_sense_adjoint): y complex64 [rows, coils, S, S] (kept: the launch works on a copy) -> fp32
    [rows, S, S].  No mask: y is zero where nothing was measured."""
    require_gpu(y, maps, out)
    if y.dtype != torch.complex64 or y.dim() != 4 or y.shape[0] < 1 or y.shape[-1] != y.shape[-2] or not kspace_size_ok(y.shape[-1]):
        raise MudiffHipError(f'sense_adjoint: y must be complex64 [rows, coils, S, S], S a power of two in [16, 512], got {y.dtype} {tuple(y.shape)}')
    rows, coils, S = int(y.shape[0]), int(y.shape[1]), int(y.shape[-1])
    maps, _ = _sense_maps('sense_adjoint', maps, rows, S)
    if maps.shape[1] != coils:
        raise MudiffHipError(f'sense_adjoint: y has {coils} coils, maps {int(maps.shape[1])}')
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != (rows, S, S) or not out.is_contiguous()):
        raise MudiffHipError(f'sense_adjoint: out must be a contiguous fp32 tensor of shape {(rows, S, S)}, got {out.dtype} {tuple(out.shape)}')
    out = torch.empty((rows, S, S), device=y.device, dtype=torch.float32) if out is None else out
    _launch('sense_adjoint', y.device, load().mud_sense_adjoint, ptr(y.clone(memory_format=torch.contiguous_format)), ptr(maps), int(maps.shape[0]), coils,
            ptr(out), rows, S, STREAM, nbytes=float(y.numel() * 40))
    return out


def sense_constrain_into(out, x_new, ahy, mask, maps, lam, iters, cg_res, work, keys_dev, seed, step, kind, t, toff, a_tab, s_tab, clean=False,
                         noise=None):
    """Unchecked launch of mud_sense_constrain into `out` (fp32, contiguous, [rows, ..., S, S]; may be x_new): GraphSampler.sample_keyed
    checks its operands once per batch, not once per step.  ahy: fp32 [rows, S, S]; mask: uint8 [1 or rows, S, S]; maps: complex64
    [1 or rows, coils, S, S]; cg_res: fp32 [rows]; work: fp32, sense_ws_floats elements; keys_dev: through check_keys and on out's device
    (None with `noise` or `clean`)."""
    rows, S, coils = out.shape[0], out.shape[-1], maps.shape[1]
    _launch('sense_constrain', out.device, load().mud_sense_constrain, ptr(x_new), ptr(ahy), ptr(mask), int(mask.shape[0]), ptr(maps), int(maps.shape[0]),
            int(coils), float(lam), int(iters), *_level_args(noise, keys_dev, seed, step, kind, t, toff, a_tab, s_tab, clean), ptr(out), ptr(cg_res),
            ptr(work), rows, S, STREAM, nbytes=float(out.numel() * (1 + int(iters)) * (40 * coils + 24)))
    return out


def sense_constrain(x_new, ahy, mask, maps, lam, iters, t, toff, a_tab, s_tab, *, noise=None, keys=None, seed=0, step=0, kind=KIND_SENSE,
                    clean=False, out=None, work=None, cg_res=None):
    """The data-consistency step of a multi-coil measurement (mud_sense_constrain).  With A x = (mask .* F(C_c x))_c, N = A^H A and
    c = clamp(t[row] + toff, 0, len(a_tab) - 1), per slice
        b = N (x_new - s_tab[c] * eta) - a_tab[c] * ahy,   (I + lam N) e = b by exactly `iters` CG steps from 0,   out = x_new - lam e
    (clean: a = 1, s = 0): the minimiser of |x - x_new|^2 + lam |A (x - s eta) - a y|^2 for ahy = sense_adjoint(y).  x_new: fp32
    [rows, S, S] or [rows, 1, S, S]; ahy: fp32 [rows, S, S]; mask, maps: as sense_measure takes them.  eta: `noise` (fp32, x_new's shape)
    when given, else the keyed normal ops.randn_keyed gives keys[r] = (slice, sample) under (seed, step, kind), drawn in the kernel.
    out: None (a new tensor), x_new (in place) or a contiguous fp32 tensor of the shape.  work: None or a contiguous fp32 workspace of
    sense_ws_floats(rows, coils, S) elements (overwritten).  cg_res: None or a contiguous fp32 [rows] tensor that receives |r_iters| / |b|
    (0 for a row whose iteration stopped early at an exact 0).  -> out, or (out, cg_res) where cg_res was given."""
    require_gpu(x_new, ahy, mask, maps, noise, t, a_tab, s_tab, out, work, cg_res)
    rows, S = _kspace_grid('sense_constrain', x_new)
    if ahy is None or ahy.dtype != torch.float32 or tuple(ahy.shape) != (rows, S, S):
        raise MudiffHipError(f'sense_constrain: ahy must be fp32 {(rows, S, S)}, got {None if ahy is None else (ahy.dtype, tuple(ahy.shape))}')
    if mask is None:
        raise MudiffHipError('sense_constrain: mask is needed')
    maps, mask = _sense_maps('sense_constrain', maps, rows, S, mask)
    lam, iters = float(lam), int(iters)
    if not (lam >= 0.0 and math.isfinite(lam)) or not 1 <= iters <= SENSE_MAX_ITERS:
        raise MudiffHipError(f'sense_constrain: lam must be finite and >= 0 and iters in [1, {SENSE_MAX_ITERS}], got {lam} and {iters}')
    x_new, noise, out = _noise_and_out('sense_constrain', x_new, noise, out)
    need = sense_ws_floats(rows, maps.shape[1], S)
    if work is not None and (work.dtype != torch.float32 or work.numel() != need or not work.is_contiguous()):
        raise MudiffHipError(f'sense_constrain: work must be a contiguous fp32 tensor of {need} elements')
    if cg_res is not None and (cg_res.dtype != torch.float32 or tuple(cg_res.shape) != (rows,) or not cg_res.is_contiguous()):
        raise MudiffHipError(f'sense_constrain: cg_res must be a contiguous fp32 [{rows}] tensor')
    t, a_tab, s_tab, kd = _level_and_keys('sense_constrain', clean, t, a_tab, s_tab, noise, keys, rows, x_new.device)
    work = torch.empty(need, device=x_new.device, dtype=torch.float32) if work is None else work
    res = torch.empty(rows, device=x_new.device, dtype=torch.float32) if cg_res is None else cg_res
    sense_constrain_into(out, x_new, ahy.contiguous(), mask, maps, lam, iters, res, work, kd, _seed64(seed), step, kind, t, toff, a_tab, s_tab, clean,
                         noise)
    return out if cg_res is None else (out, cg_res)


# columns of volume_through_plane's sums (include/mudiff_hip.h: MUD_TP_*)
TP_N_DZ, TP_S_DZ, TP_N_DZZ, TP_S_DZZ, TP_N_DX, TP_S_DX, TP_N_DY, TP_S_DY = range(8)
TP_NQ, TP_PARTS = 8, 16


def volume_through_plane(vol, mask=None, z0=0, z1=None):
    """Per-plane counts and fp64 sums of the absolute differences of a [Z, X, Y] fp32 volume (planes contiguous) along z, x and y and of
    its second difference along z, over the voxels inside the uint8 `mask` (non-zero; None: every voxel), for the planes z0..z1 clipped to
    the volume (z1 None: the last plane); planes outside that range are never read -> (device fp64 [planes, TP_NQ], first plane, last
    plane).  mud_volume_through_plane defines the columns.  Bit-identical run to run.  No synchronisation."""
    require_gpu(vol, mask)
    if vol.dtype != torch.float32 or vol.dim() != 3 or (mask is not None and (mask.dtype != torch.uint8 or mask.shape != vol.shape)):
        raise MudiffHipError(f'volume_through_plane: need an fp32 [Z, X, Y] volume and a uint8 mask of its shape (got {vol.dtype} '
                             f'{tuple(vol.shape)}' + ('' if mask is None else f', {mask.dtype} {tuple(mask.shape)}') + ')')
    Z, X, Y = vol.shape
    if min(Z, X, Y) < 1:
        raise MudiffHipError(f'volume_through_plane: empty volume {tuple(vol.shape)}')
    z0, z1 = max(0, int(z0)), Z - 1 if z1 is None else min(Z - 1, int(z1))
    if z0 > z1:
        raise MudiffHipError(f'volume_through_plane: no plane of the {Z} lies in {z0}..{z1}')
    vin, min_ = vol.contiguous(), None if mask is None else mask.contiguous()
    planes = z1 - z0 + 1
    sums = torch.empty(planes, TP_NQ, device=vol.device, dtype=torch.float64)
    ws = torch.empty(planes * TP_PARTS * TP_NQ, device=vol.device, dtype=torch.float64)
    _launch('volume_through_plane', vol.device, load().mud_volume_through_plane, ptr(vin), ptr(min_), Z, X, Y, z0, z1, ptr(sums), ptr(ws),
            ws.numel() * 8, STREAM, nbytes=float(planes) * X * Y * (5 if mask is None else 6))
    return sums, z0, z1


def ensemble_stats(samples, scale=1.0, shift=0.0, lo=-math.inf, hi=math.inf):
    """Per-pixel mean and standard deviation (N - 1) over the samples of each slice: samples [n, N, ...] (N >= 2, fp32) -> (mean, std),
    fp32 [n, ...], of y = clamp(samples*scale + shift, lo, hi); fp64 sums in sample order, so a fixed function of the samples
    (mud_ensemble_stats).  scale = shift = 0.5, [0, 1] is the pre-map of ops.to_range_0_1."""
    require_gpu(samples)
    if samples.dim() < 3:
        raise MudiffHipError(f'ensemble_stats: samples must be [n, N, ...], got {tuple(samples.shape)}')
    n, N = samples.shape[0], samples.shape[1]
    if N < 2:
        raise MudiffHipError(f'ensemble_stats: need N >= 2 samples per slice, got {N}')
    x = _f32(samples.contiguous())
    hw = x[0, 0].numel()
    mean = torch.empty(n, *x.shape[2:], device=x.device, dtype=torch.float32)
    std = torch.empty_like(mean)
    if n == 0 or hw == 0:
        return mean, std
    _launch('ensemble_stats', x.device, load().mud_ensemble_stats, ptr(x), n, N, hw, float(scale), float(shift), float(lo), float(hi),
            ptr(mean), ptr(std), STREAM, nbytes=4.0 * n * hw * (N + 2))
    return mean, std


QUANTILES_MAX_K, QUANTILES_MAX_N = 8, 64      # include/mudiff_hip.h: MUD_ENSEMBLE_MAX_QUANTILES, MUD_ENSEMBLE_QUANTILES_MAX_N


def ensemble_quantiles(samples, qs, scale=1.0, shift=0.0, lo=-math.inf, hi=math.inf, out=None):
    """Per-pixel quantiles over the samples of each slice: samples [n, N, ...] (2 <= N <= 64, fp32) and 1 to 8 fractions `qs` in [0, 1]
    -> fp32 [K, n, ...] of y = clamp(samples*scale + shift, lo, hi) (ops.ensemble_stats' pre-map): with y sorted ascending,
    h = (N - 1) q, i = min(floor(h), N - 2), out = fp32(y[i] + (h - i) * (y[i+1] - y[i])) in fp64; q = 0.5 is the median.  A pixel with
    a NaN sample gives NaN for every q.  A sorting network in registers: a fixed function of the samples (mud_ensemble_quantiles).
    `out`: a contiguous fp32 device tensor of K * n * ... elements to fill instead of a new one."""
    require_gpu(samples)
    if samples.dim() < 3:
        raise MudiffHipError(f'ensemble_quantiles: samples must be [n, N, ...], got {tuple(samples.shape)}')
    n, N = samples.shape[0], samples.shape[1]
    q = [float(v) for v in qs]
    K = len(q)
    x = _f32(samples.contiguous())
    hw = math.prod(x.shape[2:])
    shape = (K, n, *x.shape[2:])
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    else:
        require_gpu(x, out)
        if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != math.prod(shape):
            raise MudiffHipError(f'ensemble_quantiles: out must be a contiguous fp32 tensor of {math.prod(shape)} elements, got {out.dtype} '
                                 f'{tuple(out.shape)}')
        out = out.view(shape)
    if n == 0 or hw == 0:                      # nothing to launch: the entry point's own range checks, then the empty result
        if not (2 <= N <= QUANTILES_MAX_N and 1 <= K <= QUANTILES_MAX_K):
            raise MudiffHipError(f'ensemble_quantiles: need 2 to {QUANTILES_MAX_N} samples and 1 to {QUANTILES_MAX_K} quantiles, got {N} and {K}')
        return out
    _launch('ensemble_quantiles', x.device, load().mud_ensemble_quantiles, ptr(x), n, N, hw, float(scale), float(shift), float(lo),
            float(hi), (C.c_double * max(K, 1))(*q), K, ptr(out), STREAM, nbytes=4.0 * n * hw * (N + K))
    return out


# columns of volume_interval_coverage's counts and sums (include/mudiff_hip.h: MUD_VC_*)
VC_N, VC_BELOW, VC_ABOVE, VC_INSIDE, VC_NONFINITE = range(5)
VC_WIDTH, VC_WIDTH_INSIDE = range(2)
VC_NC, VC_NS, VC_PARTS = 5, 2, 16


def volume_interval_coverage(lo, hi, gt, region=None, nreg=1, z0=0, z1=None):
    """Per plane and region, how the ground truth `gt` lies to the interval [lo, hi]: three fp32 [Z, X, Y] volumes (planes contiguous)
    and the uint8 region bits of volume_metrics.region_mask (None: every voxel is in every region), for the planes z0..z1 clipped to
    the volume (z1 None: the last plane); planes outside that range are never read -> (device int64 counts [planes, nreg, VC_NC], device
    fp64 width sums [planes, nreg, VC_NS], first plane, last plane).  mud_volume_interval_coverage defines the columns: a voxel with a
    NaN in any of the three counts as VC_NONFINITE and nothing else.  Bit-identical run to run.  No synchronisation."""
    require_gpu(lo, hi, gt, region)
    vols = (lo, hi, gt)
    if any(v.dtype != torch.float32 or v.dim() != 3 or v.shape != lo.shape for v in vols) or (
            region is not None and (region.dtype != torch.uint8 or region.shape != lo.shape)):
        raise MudiffHipError('volume_interval_coverage: need three fp32 [Z, X, Y] volumes of one shape and a uint8 region volume of that '
                             'shape (got ' + ', '.join(f'{v.dtype} {tuple(v.shape)}' for v in vols + (() if region is None else (region,))) + ')')
    Z, X, Y = lo.shape
    if min(Z, X, Y) < 1:
        raise MudiffHipError(f'volume_interval_coverage: empty volume {tuple(lo.shape)}')
    nreg = int(nreg)
    if not 1 <= nreg <= VM_MAX_REGIONS:
        raise MudiffHipError(f'volume_interval_coverage: nreg must be in [1, {VM_MAX_REGIONS}], got {nreg}')
    z0, z1 = max(0, int(z0)), Z - 1 if z1 is None else min(Z - 1, int(z1))
    if z0 > z1:
        raise MudiffHipError(f'volume_interval_coverage: no plane of the {Z} lies in {z0}..{z1}')
    lo_, hi_, gt_, reg_ = lo.contiguous(), hi.contiguous(), gt.contiguous(), None if region is None else region.contiguous()
    planes = z1 - z0 + 1
    counts = torch.empty(planes, nreg, VC_NC, device=lo.device, dtype=torch.int64)
    sums = torch.empty(planes, nreg, VC_NS, device=lo.device, dtype=torch.float64)
    ws = torch.empty(planes * VC_PARTS * nreg * (VC_NC + VC_NS), device=lo.device, dtype=torch.float64)
    _launch('volume_interval_coverage', lo.device, load().mud_volume_interval_coverage, ptr(lo_), ptr(hi_), ptr(gt_), ptr(reg_), Z, X, Y, nreg,
            z0, z1, ptr(counts), ptr(sums), ptr(ws), ws.numel() * 8, STREAM, nbytes=float(planes) * X * Y * (12 if region is None else 13))
    return counts, sums, z0, z1


# ---------------------------------------------------------------------------------------------------
# --bias_correct (csrc/volume_bias.hip; the loop around these is mudiff_hip.volume_bias)
# ---------------------------------------------------------------------------------------------------
def _bias_samples(shape, shrink):
    s = max(int(shrink), 1)
    return tuple(-(-int(v) // s) for v in shape)


def _bias_volume(what, dev_raw, code, shape):
    from .volume_intake import DEVICE_DTYPES
    import numpy as np
    require_gpu(dev_raw)
    X, Y, Z = (int(v) for v in shape)
    if int(code) not in DEVICE_DTYPES:
        raise MudiffHipError(f'{what}: unsupported NIfTI datatype code {code}')
    if dev_raw.numel() != X * Y * Z or dev_raw.element_size() != np.dtype(DEVICE_DTYPES[int(code)]).itemsize or not dev_raw.is_contiguous():
        raise MudiffHipError(f'{what}: {dev_raw.numel()} voxels of {dev_raw.element_size()} bytes do not hold a {X} x {Y} x {Z} volume of '
                             f'datatype {code}')
    return X, Y, Z


def _bias_image(what, shape, shrink, *images):
    nx, ny, nz = _bias_samples(shape, shrink)
    for t in images:
        if t.dtype != torch.float32 or t.numel() != nx * ny * nz or not t.is_contiguous():
            raise MudiffHipError(f'{what}: need contiguous fp32 log images of {nx} x {ny} x {nz} samples, got {t.dtype} {tuple(t.shape)}')


def volume_bias_log(dev_raw, code, shape, slope, inter, shrink):
    """mud_volume_bias_log: the flat device array of a volume's stored voxels -> u, device fp32 [nz, ny, nx]: logf of every shrink-th
    voxel per axis, NaN where it is not finite or not > 0."""
    X, Y, Z = _bias_volume('volume_bias_log', dev_raw, code, shape)
    nx, ny, nz = _bias_samples(shape, shrink)
    u = torch.empty(nz, ny, nx, device=dev_raw.device, dtype=torch.float32)
    _launch('volume_bias_log', dev_raw.device, load().mud_volume_bias_log, ptr(dev_raw), int(code), X, Y, Z, float(slope), float(inter),
            int(shrink), ptr(u), STREAM, nbytes=float(u.numel() * (dev_raw.element_size() + 4)))
    return u


def _bias_lattices(what, lattices, levels):
    need = sum(((1 << l) + 3) ** 3 for l in range(max(int(levels), 0)))
    if lattices.dtype != torch.float64 or lattices.numel() != need or not lattices.is_contiguous():
        raise MudiffHipError(f'{what}: {levels} levels need {need} contiguous fp64 control points, got {lattices.dtype} {tuple(lattices.shape)}')


def volume_bias_corrected(u, c_old, c_new, lattices, levels, shape, shrink):
    """mud_volume_bias_corrected: c_new = float32(double(u) - F) -> device int64 [3]: the bits of the largest |c_new - c_old| and the
    order-preserving keys of the largest and the smallest finite c_new (the smallest all ones without any)."""
    require_gpu(u, c_old, c_new, lattices)
    _bias_image('volume_bias_corrected', shape, shrink, u, c_old, c_new)
    _bias_lattices('volume_bias_corrected', lattices, levels)
    X, Y, Z = (int(v) for v in shape)
    stats = torch.empty(3, device=u.device, dtype=torch.int64)
    _launch('volume_bias_corrected', u.device, load().mud_volume_bias_corrected, ptr(u), ptr(c_old), ptr(c_new), ptr(lattices), int(levels), X, Y,
            Z, int(shrink), ptr(stats), STREAM, nbytes=12.0 * u.numel())
    return stats


def volume_bias_hist(c, lo, scale, bins):
    """mud_volume_bias_hist -> device int32 [bins] (uint32 counts) of the finite values of c."""
    require_gpu(c)
    if c.dtype != torch.float32 or not c.is_contiguous():
        raise MudiffHipError(f'volume_bias_hist: need a contiguous fp32 log image, got {c.dtype}')
    hist = torch.empty(max(int(bins), 1), device=c.device, dtype=torch.int32)
    _launch('volume_bias_hist', c.device, load().mud_volume_bias_hist, ptr(c), int(c.numel()), float(lo), float(scale), int(bins), ptr(hist),
            STREAM, nbytes=4.0 * c.numel())
    return hist


def volume_bias_fit(c, table, lo, scale, level, shape, shrink, k):
    """mud_volume_bias_fit -> device int64 [2, m, m, m], m = 2^level + 3: delta and omega of one level's fit of c - table(c)."""
    require_gpu(c, table)
    _bias_image('volume_bias_fit', shape, shrink, c)
    if table.dtype != torch.float64 or not table.is_contiguous():
        raise MudiffHipError(f'volume_bias_fit: need a contiguous fp64 table, got {table.dtype}')
    X, Y, Z = (int(v) for v in shape)
    m = (1 << min(max(int(level), 0), 8)) + 3
    sums = torch.empty(2, m, m, m, device=c.device, dtype=torch.int64)
    _launch('volume_bias_fit', c.device, load().mud_volume_bias_fit, ptr(c), ptr(table), int(table.numel()), float(lo), float(scale), int(level),
            X, Y, Z, int(shrink), int(k), ptr(sums), STREAM, nbytes=4.0 * c.numel())
    return sums


def volume_bias_apply(dev_raw, code, shape, slope, inter, lattices, levels, field=False):
    """mud_volume_bias_apply -> device fp32 [Z, Y, X]: every voxel / exp(F) (with `field`: exp(F) itself)."""
    X, Y, Z = _bias_volume('volume_bias_apply', dev_raw, code, shape)
    require_gpu(dev_raw, lattices)
    _bias_lattices('volume_bias_apply', lattices, levels)
    out = torch.empty(Z, Y, X, device=dev_raw.device, dtype=torch.float32)
    _launch('volume_bias_apply', dev_raw.device, load().mud_volume_bias_apply, ptr(dev_raw), int(code), X, Y, Z, float(slope), float(inter),
            ptr(lattices), int(levels), int(bool(field)), ptr(out), STREAM, nbytes=float(out.numel() * (dev_raw.element_size() + 4)))
    return out


# ---------------------------------------------------------------------------------------------------
# --denoise (csrc/volume_denoise.hip; the host's share is mudiff_hip.volume_denoise)
# ---------------------------------------------------------------------------------------------------
def volume_denoise_residual(dev_raw, code, shape, slope, inter):
    """mud_volume_denoise_residual: the flat device array of a volume's stored voxels -> device int32 [Z, Y, X]: the uint32 bits of the
    pseudo-residual |eps| of every voxel of the estimation set, all ones elsewhere."""
    X, Y, Z = _bias_volume('volume_denoise_residual', dev_raw, code, shape)
    keys = torch.empty(Z, Y, X, device=dev_raw.device, dtype=torch.int32)
    _launch('volume_denoise_residual', dev_raw.device, load().mud_volume_denoise_residual, ptr(dev_raw), int(code), X, Y, Z, float(slope),
            float(inter), ptr(keys), STREAM, nbytes=float(keys.numel() * (dev_raw.element_size() + 4)))
    return keys


def volume_denoise_select_hist(keys, prefix, which):
    """mud_volume_denoise_select_hist -> device int32 [256] (uint32 counts): pass `which` (0 .. 3) of the radix select over the keys
    whose higher bytes are `prefix`."""
    require_gpu(keys)
    if keys.dtype != torch.int32 or not keys.is_contiguous() or keys.numel() == 0:
        raise MudiffHipError(f'volume_denoise_select_hist: need contiguous 32-bit keys, got {keys.dtype} {tuple(keys.shape)}')
    hist = torch.empty(256, device=keys.device, dtype=torch.int32)
    _launch('volume_denoise_select_hist', keys.device, load().mud_volume_denoise_select_hist, ptr(keys), int(keys.numel()), int(prefix),
            int(which), ptr(hist), STREAM, nbytes=4.0 * keys.numel())
    return hist


def volume_denoise_nlm(dev_raw, code, shape, slope, inter, search, patch, sigma, beta, rician=False):
    """mud_volume_denoise_nlm -> (device fp32 [Z, Y, X]: the non-local-means estimate of every voxel; device int32 [1]: how many voxels
    that were not 0 came out 0)."""
    X, Y, Z = _bias_volume('volume_denoise_nlm', dev_raw, code, shape)
    out = torch.empty(Z, Y, X, device=dev_raw.device, dtype=torch.float32)
    zeroed = torch.empty(1, device=dev_raw.device, dtype=torch.int32)
    side, box = 2 * int(search) + 1, 2 * int(patch) + 1
    _launch('volume_denoise_nlm', dev_raw.device, load().mud_volume_denoise_nlm, ptr(dev_raw), int(code), X, Y, Z, float(slope), float(inter),
            int(search), int(patch), float(sigma), float(beta), int(bool(rician)), ptr(out), ptr(zeroed), STREAM,
            flops=2.0 * out.numel() * (side ** 3 - 1) * box ** 3, nbytes=float(out.numel() * (dev_raw.element_size() + 4)))
    return out, zeroed


# ---------------------------------------------------------------------------------------------------
# --unring (csrc/volume_unring.hip; the host's share, the tables, is mudiff_hip.volume_unring)
# ---------------------------------------------------------------------------------------------------
def volume_unring_filter(dev_raw, code, shape, slope, inter, axes, twiddle, kernel):
    """mud_volume_unring_filter -> (ix, iy: device fp32 [Z, Y, X], ix + iy = the volume with its non-finite voxels read as 0; device int32
    [1] (uint32): how many those were).  twiddle, kernel: the device tables of volume_unring.filter_tables(nx, ny)."""
    X, Y, Z = _bias_volume('volume_unring_filter', dev_raw, code, shape)
    require_gpu(dev_raw, twiddle, kernel)
    ax, ay = (int(a) for a in axes)
    if not (0 <= ax <= 2 and 0 <= ay <= 2 and ax != ay):
        raise MudiffHipError(f'volume_unring_filter: two distinct storage axes in [0, 2], got {ax} and {ay}')
    nx, ny = (X, Y, Z)[ax], (X, Y, Z)[ay]
    for t, count, what in ((twiddle, 2 * nx, 'twiddle'), (kernel, (nx // 2 + 1) * ny, 'kernel')):
        if t.dtype != torch.float64 or t.numel() != count or not t.is_contiguous():
            raise MudiffHipError(f'volume_unring_filter: need {count} contiguous fp64 entries of the {what} table, got {t.dtype} {tuple(t.shape)}')
    ix = torch.empty(Z, Y, X, device=dev_raw.device, dtype=torch.float32)
    iy = torch.empty_like(ix)
    nonfinite = torch.empty(1, device=dev_raw.device, dtype=torch.int32)
    _launch('volume_unring_filter', dev_raw.device, load().mud_volume_unring_filter, ptr(dev_raw), int(code), X, Y, Z, float(slope), float(inter),
            ax, ay, ptr(twiddle), ptr(kernel), ptr(ix), ptr(iy), ptr(nonfinite), STREAM,
            flops=2.0 * ix.numel() * (3.0 * nx + 2.0 * ny), nbytes=float(ix.numel() * (2 * dev_raw.element_size() + 32)))
    return ix, iy, nonfinite


def volume_unring_lines(vol, shape, axis, normal, shifts, window, table, out=None, accumulate=False, jmap=False):
    """mud_volume_unring_lines on the fp32 [Z, Y, X] device volume `vol` -> (out, jmap or None, device int64 [2]: the voxels that moved and
    the sum of their |shift| in units of 1 / (2 shifts + 1)).  out: where the result goes (`vol` itself by default: in place), added to
    what it holds with `accumulate`; jmap=True also returns the int8 [Z, Y, X] map of the chosen shifts."""
    require_gpu(vol, table)
    X, Y, Z = _fg_grid('volume_unring_lines', vol, shape, torch.float32)
    out = vol if out is None else out
    _fg_grid('volume_unring_lines', out, shape, torch.float32)
    n = (X, Y, Z)[int(axis)] if 0 <= int(axis) <= 2 else 0
    a, b = (int(w) for w in window)
    if table.dtype != torch.float32 or table.numel() != (2 * int(shifts) + 1) * n or not table.is_contiguous():
        raise MudiffHipError(f'volume_unring_lines: need the contiguous fp32 table of {2 * int(shifts) + 1} shifts of {n} voxels, got {table.dtype} '
                             f'{tuple(table.shape)}')
    chosen = torch.empty(Z, Y, X, device=vol.device, dtype=torch.int8) if jmap else None
    counters = torch.empty(2, device=vol.device, dtype=torch.int64)
    _launch('volume_unring_lines', vol.device, load().mud_volume_unring_lines, ptr(vol), X, Y, Z, int(axis), int(normal), int(shifts), a, b, ptr(table),
            ptr(out), int(bool(accumulate)), ptr(chosen) if jmap else None, ptr(counters), STREAM,
            flops=2.0 * vol.numel() * n * 2 * int(shifts), nbytes=8.0 * vol.numel())
    return out, chosen, counters


# ---------------------------------------------------------------------------------------------------
# --foreground (csrc/volume_foreground.hip; the host's share is mudiff_hip.volume_foreground)
# ---------------------------------------------------------------------------------------------------
def _fg_grid(what, t, shape, dtype):
    require_gpu(t)
    X, Y, Z = (int(v) for v in shape)
    if t.dtype != dtype or t.numel() != X * Y * Z or not t.is_contiguous():
        raise MudiffHipError(f'{what}: need a contiguous {dtype} volume of {X} x {Y} x {Z} voxels, got {t.dtype} {tuple(t.shape)}')
    return X, Y, Z


def volume_fg_range(dev_raw, code, shape, slope, inter):
    """mud_volume_fg_range -> device int32 [3] (uint32): the largest ~key and the largest key of the candidates (the finite voxels that
    are != 0) and their number (volume_foreground.range_of decodes them)."""
    X, Y, Z = _bias_volume('volume_fg_range', dev_raw, code, shape)
    out = torch.empty(3, device=dev_raw.device, dtype=torch.int32)
    _launch('volume_fg_range', dev_raw.device, load().mud_volume_fg_range, ptr(dev_raw), int(code), X, Y, Z, float(slope), float(inter), ptr(out),
            STREAM, nbytes=float(dev_raw.numel() * dev_raw.element_size()))
    return out


def volume_fg_hist(dev_raw, code, shape, slope, inter, lo, scale, bins):
    """mud_volume_fg_hist -> device int32 [bins] (uint32 counts) of the candidates."""
    X, Y, Z = _bias_volume('volume_fg_hist', dev_raw, code, shape)
    hist = torch.empty(max(int(bins), 1), device=dev_raw.device, dtype=torch.int32)
    _launch('volume_fg_hist', dev_raw.device, load().mud_volume_fg_hist, ptr(dev_raw), int(code), X, Y, Z, float(slope), float(inter), float(lo),
            float(scale), int(bins), ptr(hist), STREAM, nbytes=float(dev_raw.numel() * dev_raw.element_size()))
    return hist


def volume_fg_mask(dev_raw, code, shape, slope, inter, lo, scale, bins, k):
    """mud_volume_fg_mask -> device uint8 [Z, Y, X]: 1 for a candidate whose bin is above k."""
    X, Y, Z = _bias_volume('volume_fg_mask', dev_raw, code, shape)
    mask = torch.empty(Z, Y, X, device=dev_raw.device, dtype=torch.uint8)
    _launch('volume_fg_mask', dev_raw.device, load().mud_volume_fg_mask, ptr(dev_raw), int(code), X, Y, Z, float(slope), float(inter), float(lo),
            float(scale), int(bins), int(k), ptr(mask), STREAM, nbytes=float(dev_raw.numel() * (dev_raw.element_size() + 1)))
    return mask


def volume_fg_morph(mask, shape, dilate):
    """mud_volume_fg_morph -> device uint8 [Z, Y, X]: one erosion (dilate False) or one dilation of the mask over the 6-neighbourhood."""
    X, Y, Z = _fg_grid('volume_fg_morph', mask, shape, torch.uint8)
    out = torch.empty(Z, Y, X, device=mask.device, dtype=torch.uint8)
    _launch('volume_fg_morph', mask.device, load().mud_volume_fg_morph, ptr(mask), X, Y, Z, int(bool(dilate)), ptr(out), STREAM,
            nbytes=2.0 * mask.numel())
    return out


def volume_fg_label(mask, shape, value):
    """mud_volume_fg_label -> device int32 [Z, Y, X]: the smallest linear index of the 6-connected component of every voxel whose mask
    is `value` (0 or 1), -1 elsewhere."""
    X, Y, Z = _fg_grid('volume_fg_label', mask, shape, torch.uint8)
    labels = torch.empty(Z, Y, X, device=mask.device, dtype=torch.int32)
    _launch('volume_fg_label', mask.device, load().mud_volume_fg_label, ptr(mask), X, Y, Z, int(value), ptr(labels), STREAM,
            nbytes=14.0 * mask.numel())
    return labels


def volume_fg_census(labels, shape):
    """mud_volume_fg_census -> (device int32 [X*Y*Z] (uint32): per root the voxel count, bit 31 set for a component on a face of the
    volume; device int64 [2] (uint64): the winner (count << 32) | (0xFFFFFFFF - root) and the number of components)."""
    X, Y, Z = _fg_grid('volume_fg_census', labels, shape, torch.int32)
    census = torch.empty(X * Y * Z, device=labels.device, dtype=torch.int32)
    summary = torch.empty(2, device=labels.device, dtype=torch.int64)
    _launch('volume_fg_census', labels.device, load().mud_volume_fg_census, ptr(labels), X, Y, Z, ptr(census), ptr(summary), STREAM,
            nbytes=16.0 * labels.numel())
    return census, summary


def volume_fg_select(labels, census, root, holes, mask=None):
    """mud_volume_fg_select -> (mask, device int32 [1]: the voxels switched on).  holes False: a new mask, 1 where the label is `root`;
    holes True: `mask` itself, with every labelled component that does not touch a face (census) switched on."""
    require_gpu(labels, census, mask)
    if labels.dtype != torch.int32 or not labels.is_contiguous() or labels.numel() == 0:
        raise MudiffHipError(f'volume_fg_select: need contiguous int32 labels, got {labels.dtype} {tuple(labels.shape)}')
    if holes:
        if mask is None or mask.dtype != torch.uint8 or mask.numel() != labels.numel() or not mask.is_contiguous():
            raise MudiffHipError('volume_fg_select: filling the holes needs the uint8 mask the complement was labelled from')
        if census is None or census.dtype != torch.int32 or census.numel() != labels.numel() or not census.is_contiguous():
            raise MudiffHipError('volume_fg_select: filling the holes needs the census of the labels')
    else:
        mask = torch.empty(labels.shape, device=labels.device, dtype=torch.uint8)
    count = torch.empty(1, device=labels.device, dtype=torch.int32)
    _launch('volume_fg_select', labels.device, load().mud_volume_fg_select, ptr(labels), ptr(census), int(labels.numel()), int(root),
            int(bool(holes)), ptr(mask), ptr(count), STREAM, nbytes=5.0 * labels.numel())
    return mask, count


def volume_fg_apply(dev_raw, code, shape, slope, inter, mask):
    """mud_volume_fg_apply -> (device fp32 [Z, Y, X]: the voxel inside the mask, +0 outside; device int32 [1]: the candidates outside)."""
    X, Y, Z = _bias_volume('volume_fg_apply', dev_raw, code, shape)
    _fg_grid('volume_fg_apply', mask, shape, torch.uint8)
    require_gpu(dev_raw, mask)
    out = torch.empty(Z, Y, X, device=dev_raw.device, dtype=torch.float32)
    removed = torch.empty(1, device=dev_raw.device, dtype=torch.int32)
    _launch('volume_fg_apply', dev_raw.device, load().mud_volume_fg_apply, ptr(dev_raw), int(code), X, Y, Z, float(slope), float(inter), ptr(mask),
            ptr(out), ptr(removed), STREAM, nbytes=float(out.numel() * (dev_raw.element_size() + 5)))
    return out, removed


# ---------------------------------------------------------------------------------------------------
# --brain_extract (csrc/volume_brain.hip; the host's share is mudiff_hip.volume_brain)
# ---------------------------------------------------------------------------------------------------
def volume_edt(mask, shape, value, spacing):
    """mud_volume_edt -> device fp64 [Z, Y, X]: the squared distance, in the units of spacing = (sx, sy, sz), from every voxel to the
    nearest voxel whose mask is `value` (0 or 1); +inf everywhere without one."""
    X, Y, Z = _fg_grid('volume_edt', mask, shape, torch.uint8)
    sx, sy, sz = (float(v) for v in spacing)
    d2 = torch.empty(Z, Y, X, device=mask.device, dtype=torch.float64)
    _launch('volume_edt', mask.device, load().mud_volume_edt, ptr(mask), X, Y, Z, int(value), sx, sy, sz, ptr(d2), STREAM,
            nbytes=41.0 * mask.numel())
    return d2


def volume_edt_select(d2, r2, above, within=None):
    """mud_volume_edt_select -> (device uint8 mask shaped like d2: (d2 > r2 if above else d2 <= r2) and within; device int32 [1]: the
    voxels switched on)."""
    require_gpu(d2, within)
    if d2.dtype != torch.float64 or not d2.is_contiguous() or d2.numel() == 0:
        raise MudiffHipError(f'volume_edt_select: need contiguous fp64 squared distances, got {d2.dtype} {tuple(d2.shape)}')
    if within is not None and (within.dtype != torch.uint8 or within.numel() != d2.numel() or not within.is_contiguous()):
        raise MudiffHipError(f'volume_edt_select: `within` must be a contiguous uint8 mask of {d2.numel()} voxels')
    out = torch.empty(d2.shape, device=d2.device, dtype=torch.uint8)
    count = torch.empty(1, device=d2.device, dtype=torch.int32)
    _launch('volume_edt_select', d2.device, load().mud_volume_edt_select, ptr(d2), int(d2.numel()), float(r2), int(bool(above)), ptr(within),
            ptr(out), ptr(count), STREAM, nbytes=10.0 * d2.numel())
    return out, count


# ---------------------------------------------------------------------------------------------------
# --reorient (csrc/volume_reorient.hip; the host's share is mudiff_hip.volume_reorient)
# ---------------------------------------------------------------------------------------------------
def volume_reorient(dev_flat, elem_bytes, shape, plan):
    """mud_volume_reorient: the flat device array of a volume's voxels (x fastest, `shape` = (SX, SY, SZ), elements of `elem_bytes`
    bytes) -> a flat device tensor of the same dtype holding the volume with its storage axes permuted and flipped by `plan`
    (volume_reorient.ReorientPlan, or anything with `perm` and `flip`): dst[i0, i1, i2] = src[j], j[perm[o]] = S[perm[o]] - 1 - i_o
    if flip[o] else i_o.  The destination's extents are plan.shape = (S[perm[0]], S[perm[1]], S[perm[2]])."""
    require_gpu(dev_flat)
    SX, SY, SZ = (int(v) for v in shape)
    if dev_flat.dim() != 1 or dev_flat.numel() != SX * SY * SZ or dev_flat.element_size() != int(elem_bytes) or not dev_flat.is_contiguous():
        raise MudiffHipError(f'volume_reorient: {tuple(dev_flat.shape)} elements of {dev_flat.element_size()} bytes do not hold a flat '
                             f'{SX} x {SY} x {SZ} volume of {elem_bytes}-byte elements')
    p0, p1, p2 = (int(v) for v in plan.perm)
    mask = sum(1 << o for o, f in enumerate(plan.flip) if f)
    out = torch.empty_like(dev_flat)
    _launch('volume_reorient', dev_flat.device, load().mud_volume_reorient, ptr(dev_flat), int(elem_bytes), SX, SY, SZ, p0, p1, p2, mask, ptr(out),
            STREAM, nbytes=2.0 * dev_flat.numel() * dev_flat.element_size())
    return out


# ---------------------------------------------------------------------------------------------------
# --antialias / --conform (csrc/volume_lowpass.hip; the host's share is mudiff_hip.volume_conform)
# ---------------------------------------------------------------------------------------------------
def volume_lowpass(dev_raw, code, shape, slope, inter, weights_xyz, out=None, scratch=None):
    """mud_volume_lowpass: the flat device array of a volume's stored voxels (datatype `code`, shape (X, Y, Z)) -> (device fp32 [Z,Y,X]:
    the volume after one Gaussian pass along every axis that has weights, the non-finite voxels that were read as 0).  weights_xyz:
    per axis None (not filtered) or the 2 R + 1 host weights w[t + R] (volume_conform.weights).  Without any weights nothing is launched:
    (None, 0), and the caller goes on with the stored voxels.  `out` / `scratch`: fp32 volumes to use instead of fresh ones."""
    X, Y, Z = _bias_volume('volume_lowpass', dev_raw, code, shape)
    if len(weights_xyz) != 3:
        raise ValueError(f'volume_lowpass: need the weights of three axes, got {len(weights_xyz)}')
    arrays, args = [], []
    for w in weights_xyz:
        if w is None:
            args += [None, 0]
            continue
        w = np.ascontiguousarray(np.asarray(w, np.float64).reshape(-1))
        if w.size % 2 != 1:
            raise ValueError(f'volume_lowpass: 2 R + 1 weights per axis, got {w.size}')
        arrays.append(w)                                   # (kept alive until the call has returned)
        args += [w.ctypes.data_as(C.POINTER(C.c_double)), w.size // 2]
    if not arrays:
        return None, 0
    if out is None:
        out = torch.empty(Z, Y, X, device=dev_raw.device, dtype=torch.float32)
    if scratch is None and len(arrays) > 1:
        scratch = torch.empty(Z, Y, X, device=dev_raw.device, dtype=torch.float32)
    require_gpu(dev_raw, out, scratch)
    bad = torch.empty(1, device=dev_raw.device, dtype=torch.int32)
    _launch('volume_lowpass', dev_raw.device, load().mud_volume_lowpass, ptr(dev_raw), int(code), X, Y, Z, float(slope), float(inter), *args,
            ptr(out), ptr(scratch), ptr(bad), STREAM, nbytes=float(dev_raw.numel() * (dev_raw.element_size() + 4 + 8 * (len(arrays) - 1))))
    return out, int(bad.cpu().numpy().view(np.uint32)[0])


# ---------------------------------------------------------------------------------------------------
# --align (csrc/volume_align.hip; the host's share is mudiff_hip.volume_align)
# ---------------------------------------------------------------------------------------------------
def volume_mirror_moments(dev_raw, code, shape, slope, inter, mats, stride, lo, scale, bins):
    """mud_volume_mirror_moments: the flat device array of a volume's stored voxels and K candidate matrices (host, [K, 3, 4] or [K, 12]
    fp64: voxel index -> the voxel coordinate of its mirror image) -> device int64 [K, 6] (uint64 sums): n, sum a, sum b, sum a^2, sum b^2,
    sum a b of the bin indices over the overlap, one launch for all K.  ValueError, before anything is uploaded or launched, for matrices
    that are not finite."""
    X, Y, Z = _bias_volume('volume_mirror_moments', dev_raw, code, shape)
    m = np.ascontiguousarray(np.asarray(mats, np.float64).reshape(-1, 12))
    if m.shape[0] < 1 or not np.isfinite(m).all():
        raise ValueError(f'volume_mirror_moments: need at least one candidate and finite matrices, got {m.shape[0]} candidates')
    K = int(m.shape[0])
    dev_m = torch.from_numpy(m).to(dev_raw.device)
    sums = torch.empty(K, 6, device=dev_raw.device, dtype=torch.int64)
    _launch('volume_mirror_moments', dev_raw.device, load().mud_volume_mirror_moments, ptr(dev_raw), int(code), X, Y, Z, float(slope), float(inter),
            ptr(dev_m), K, int(stride), float(lo), float(scale), int(bins), ptr(sums), STREAM,
            nbytes=float(dev_raw.numel() * dev_raw.element_size()) / max(int(stride), 1) ** 3 * 9.0 * K)
    return sums
