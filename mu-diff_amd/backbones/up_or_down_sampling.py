"""StyleGAN2-style FIR resampling front ends (reference backbones/up_or_down_sampling.py) over the
gfx950 up-FIR-down kernel.  Public functions keep the reference's names, arguments and NCHW tensors."""
import numpy as np
import torch
import torch.nn as nn

from mudiff_hip import ops
from mudiff_hip.ops import View
from utils.op import upfirdn2d


def _setup_kernel(k):
    k = np.asarray(k, dtype=np.float32)
    if k.ndim == 1:
        k = np.outer(k, k)
    k /= np.sum(k)
    assert k.ndim == 2 and k.shape[0] == k.shape[1]
    return k


def fir_params(mode, k=None, factor=2, gain=1, conv_k=3):
    """(kernel2d, up, down, (pad0, pad1)) for 'up' (upsample_2d:200-229), 'down' (downsample_2d:232-262)
    and 'conv_down' (the FIR stage of conv_downsample_2d:149-183)."""
    if k is None:
        k = [1] * factor
    if mode == 'up':
        kk = _setup_kernel(k) * (gain * (factor ** 2))
        p = kk.shape[0] - factor
        return kk, factor, 1, ((p + 1) // 2 + factor - 1, p // 2)
    if mode == 'naive_up':       # nearest-neighbour repeat (naive_upsample_2d:64-68): ones(f,f), zero-stuffed input, pad (f-1, 0)
        return np.ones((factor, factor), np.float32), factor, 1, (factor - 1, 0)
    if mode == 'naive_down':     # box mean (naive_downsample_2d:71-74)
        return np.full((factor, factor), 1.0 / (factor * factor), np.float32), 1, factor, (0, 0)
    kk = _setup_kernel(k) * gain
    if mode == 'down':
        p = kk.shape[0] - factor
        return kk, 1, factor, ((p + 1) // 2, p // 2)
    if mode == 'conv_down':
        p = (kk.shape[0] - factor) + (conv_k - 1)
        return kk, 1, 1, ((p + 1) // 2, p // 2)
    raise ValueError(mode)


_DEV_KERNELS = {}


def _device_kernel(kk, device):
    """FIR taps as a cached device tensor (no host->device copy per call, so hipGraph capture works)."""
    key = (kk.tobytes(), kk.shape, str(device))
    t = _DEV_KERNELS.get(key)
    if t is None:
        t = torch.tensor(kk, device=device, dtype=torch.float32)
        _DEV_KERNELS[key] = t
    return t


def upsample_2d(x, k=None, factor=2, gain=1):
    kk, up, down, pad = fir_params('up', k, factor, gain)
    return upfirdn2d(x, torch.tensor(kk, device=x.device, dtype=x.dtype), up=up, pad=pad)


def downsample_2d(x, k=None, factor=2, gain=1):
    kk, up, down, pad = fir_params('down', k, factor, gain)
    return upfirdn2d(x, torch.tensor(kk, device=x.device, dtype=x.dtype), down=down, pad=pad)


def conv_downsample_2d(x, w, k=None, factor=2, gain=1):
    """FIR (padded once) then the strided convolution with OIHW weights `w`, no bias."""
    kk, _, _, pad = fir_params('conv_down', k, factor, gain, conv_k=w.shape[-1])
    xf = upfirdn2d(x, torch.tensor(kk, device=x.device, dtype=x.dtype), pad=pad)
    out = ops.conv(View.from_nchw(xf), ops.direct_weight(w), w.shape[-1], w.shape[0], mfma=False, stride=factor, pad=0)
    return out.to_nchw()


def naive_upsample_2d(x, factor=2):
    """Nearest-neighbour repeat (reference :64-68) on the same up-FIR-down kernel: exact (one tap of weight 1)."""
    kk, up, down, pad = fir_params('naive_up', factor=factor)
    return upfirdn2d(x, _device_kernel(kk, x.device), up=up, pad=pad)


def naive_downsample_2d(x, factor=2):
    """factor x factor box mean (reference :71-74)."""
    kk, up, down, pad = fir_params('naive_down', factor=factor)
    return upfirdn2d(x, _device_kernel(kk, x.device), down=down, pad=pad)


def resample_view(x: View, direction, fir, fir_kernel):
    """Parameter-free x2 resampling of an NHWC view (Upsample / Downsample with_conv=False): the single-channel image
    pyramids go through the planes kernel (NHWC == planes when C == 1), feature maps through the NHWC kernel."""
    kk, up, down, pad = fir_params(direction if fir else 'naive_' + direction, fir_kernel)
    if x.C % 4 == 0:
        return ops.fir_nhwc(x, kk, up, down, pad)[0]
    assert x.ld == x.C, 'planes path needs a dense view'
    t = x.base.reshape(x.B, x.H, x.W, x.C)
    planes = t.reshape(x.B, 1, x.H, x.W) if x.C == 1 else t.permute(0, 3, 1, 2).contiguous()
    r = upfirdn2d(planes, _device_kernel(kk, x.device), up=up, down=down, pad=pad)
    return View.from_nchw(r)


def fold_fir_conv_weight(w, k1d, dtype=torch.float32):
    """The weights of the ONE convolution that a separable 4x4 FIR (1-D taps `k1d`, gain included, pad (2, 2)) followed by a 3x3
    stride-2 pad-0 convolution `w` [Cout,Cin,3,3] is: W6 = w (*) k, a 6x6 stride-2 pad-2 convolution - written as the 3x3 stride-1
    pad-1 convolution over the 2x2 space-to-depth view of the input that mud_conv_args.in_s2d gathers: [Cout, 4 Cin, 3, 3], view
    channel (py*2 + px)*Cin + c, tap (jy + 1, jx + 1) = W6[2 jy + py + 2, 2 jx + px + 2].  Composed in fp64, rounded once to `dtype`.
    (upfirdn2d correlates with the FLIPPED kernel, hence kf below.)"""
    Cout, Cin = w.shape[:2]
    kf = torch.as_tensor(np.asarray(k1d, dtype=np.float64)[::-1].copy(), device=w.device)        # FIR as a correlation: flipped taps
    w64 = w.detach().double()
    # out[Y] = sum_a w[a] fir[2Y + a], fir[i] = sum_t kf[t] xpad[i + t], xpad[j] = x[j - 2]  ->  W6[u] = sum_{a + t = u} w[a] kf[t], x index 2Y + u - 2
    w6 = torch.zeros(Cout, Cin, 6, 6, dtype=torch.float64, device=w.device)
    for a in range(3):
        for b in range(3):
            w6[:, :, a:a + 4, b:b + 4] += w64[:, :, a, b, None, None] * (kf[:, None] * kf[None, :])
    # u = 2 (jy + 1) + py: [Cout, Cin, jy, py, jx, px] -> [Cout, py, px, Cin, jy, jx]
    folded = w6.reshape(Cout, Cin, 3, 2, 3, 2).permute(0, 3, 5, 1, 2, 4).reshape(Cout, 4 * Cin, 3, 3)
    return folded.to(dtype).contiguous()


def fold_weight_exponent(w):
    """The power-of-two pre-scale of a folded operand: the e with max|w| * 2^e in (128, 256] (0 for an all-zero or non-finite w)."""
    m = float(w.detach().abs().max())
    if not (m > 0.0) or not np.isfinite(m):
        return 0
    return max(-60, min(60, 8 - int(np.ceil(np.log2(m)))))


def separable_taps(kk, pad):
    """The 1-D taps t of a 4x4 FIR that is exactly t (x) t in fp64, padded (2, 2) - the filter fold_fir_conv_weight takes - or None."""
    k = np.asarray(kk, dtype=np.float64)
    if k.shape != (4, 4) or tuple(pad) != (2, 2) or not k.sum() > 0.0:
        return None
    t = k.sum(axis=1) / np.sqrt(k.sum())
    return t if np.allclose(np.outer(t, t), k, rtol=1e-7, atol=0.0) else None


def padded_strided_conv(x: View, kk, pad, weights, ks, cout, bias, res, out_scale, out, layer=None, folded=None):
    """FIR `kk` with padding `pad` (an identity tap = pure zero padding), then a stride-2 pad-0 ks x ks conv whose
    epilogue adds bias / residual and rescales.  `weights(mfma, prec)` returns the packed (for plan `prec`) or direct-layout
    weights; `layer`: the launch's name in a launch record.  `folded(prec)`, when given, returns (packed weights, w_exp) of the same
    operator as ONE 3x3 stride-1 convolution over the 2x2 space-to-depth view of x (fold_fir_conv_weight): taken where the
    library has that launch (ops.in_s2d_ok) - the FIR launch and the padded tensor are gone; knob MUD_PYR_S2D."""
    if x.C % 4 == 0 and x.C >= 8 and ks == 3 and x.H % 2 == 0 and x.W % 2 == 0:
        if folded is not None and ops.PYR_S2D:
            # the plan of the sub2 launch this replaces: fp16 x 3 under 'auto' / 'off' / 'all', single-pass under 'fp16'
            prec = ops.PREC_16X1 if ops.PREC_PLAN == 'fp16' else ops.PREC_16X3
            if ops.in_s2d_ok(x.B, x.H, x.W, x.C, cout, prec):
                wf, w_exp = folded(prec)
                return ops.conv(x, wf, 3, cout, mfma=True, bias=bias, res=res, out_scale=out_scale, out=out, in_s2d=True, prec=prec, w_exp=w_exp,
                                layer=layer, flops=2.0 * x.B * (x.H // 2) * (x.W // 2) * cout * x.C * 9)      # (the stride-2 conv's algorithmic count)
        # matrix-core path: the stride-2 pad-0 conv of the padded (H+1)x(W+1) image is the odd-position subset
        # of the stride-1 pad-1 conv (4x the MFMA work, still ~5x faster than the direct kernel)
        xf, _ = ops.fir_nhwc(x, kk, 1, 1, pad)
        prec = ops.choose_prec(xf, cout, ops.PRO_NONE, sub2=True)       # (only the single-pass plan has a sub2 form)
        return ops.conv(xf, weights(True, prec), 3, cout, mfma=True, bias=bias, res=res, out_scale=out_scale, out=out, sub2=True, prec=prec,
                        layer=layer)
    if x.C % 4 == 0:
        xf, _ = ops.fir_nhwc(x, kk, 1, 1, pad)
    else:   # image pyramid with few channels: planes kernel
        assert x.ld == x.C
        t = x.base.reshape(x.B, x.H, x.W, x.C)
        planes = t.reshape(x.B, 1, x.H, x.W) if x.C == 1 else t.permute(0, 3, 1, 2).contiguous()
        xf = View.from_nchw(upfirdn2d(planes, _device_kernel(np.ascontiguousarray(kk, np.float32), x.device), pad=pad))
    return ops.conv(xf, weights(False), ks, cout, mfma=False, stride=2, pad=0, bias=bias, res=res, out_scale=out_scale, out=out)


class Conv2d(nn.Module):
    """Conv2d with optional FIR down-sampling (reference up_or_down_sampling.py:28-61).  `up=True` is
    dead code in the reference (its upsample_conv_2d raises on torch tensors)."""

    def __init__(self, in_ch, out_ch, kernel, up=False, down=False, resample_kernel=(1, 3, 3, 1), use_bias=True, kernel_init=None):
        super().__init__()
        assert not (up and down)
        assert kernel >= 1 and kernel % 2 == 1
        self.weight = nn.Parameter(torch.zeros(out_ch, in_ch, kernel, kernel))
        if kernel_init is not None:
            self.weight.data = kernel_init(self.weight.data.shape)
        if use_bias:
            self.bias = nn.Parameter(torch.zeros(out_ch))
        self.up, self.down, self.resample_kernel, self.kernel, self.use_bias = up, down, resample_kernel, kernel, use_bias
        self._prep = None
        self._fold = None
        # down-sampling 3x3 with a separable 4x4 FIR: the 1-D taps the folded launch composes its weights from (else None), decided once
        self._fold_taps = None
        if down and kernel == 3:
            kk, _, _, pad = fir_params('conv_down', resample_kernel, conv_k=kernel)
            self._fold_taps = separable_taps(kk, pad)

    def _weights(self, mfma=False, prec=ops.PREC_16X3):
        key = (self.weight._version, self.weight.data_ptr(), mfma, prec)
        if self._prep is None or self._prep[0] != key:
            with torch.no_grad():
                self._prep = (key, ops.pack_conv_weight(self.weight, prec=prec) if mfma else ops.direct_weight(self.weight))
        return self._prep[1]

    def _folded_weights(self, prec):
        """Down-sampling 3x3 only: FIR and stride-2 convolution composed into one 3x3 operand over the space-to-depth view, once per
        weight version (fold_fir_conv_weight), packed for plan `prec` -> (packed, w_exp).  The composed taps carry the FIR's 1/64 ... 9/64:
        next to O(1) activations their fp16 lo pieces (2^-11 of a tap) fall below fp16's smallest subnormal step, so the operand is
        packed as W * 2^w_exp with the largest tap in (128, 256] - a power of two, exact - and the launch takes it back out of the sum
        (mud_conv_args.in_s2d).  One host sync (the largest tap), at pack time only - so never under graph capture: the eager pass
        that every capture follows packs the operand, and a weight that changed since then is an error there, not a silent sync."""
        key = (self.weight._version, self.weight.data_ptr(), prec)
        if self._fold is None or self._fold[0] != key:
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('Conv2d: the folded down-sampling operand must be packed before graph capture (run the layer once eagerly)')
            with torch.no_grad():
                w64 = fold_fir_conv_weight(self.weight, self._fold_taps, dtype=torch.float64)
                w_exp = fold_weight_exponent(w64)
                self._fold = (key, (ops.pack_conv_weight((w64 * 2.0 ** w_exp).float(), prec=prec), w_exp))
        return self._fold[1]

    def run(self, x: View, res: View = None, out_scale=1.0, out: View = None):
        """NHWC entry used by the generators; residual add and rescale fused into the conv epilogue."""
        if self.up:
            raise NotImplementedError('Conv2d(up=True) is unreachable in the reference (upsample_conv_2d raises)')
        bias = self.bias.detach() if self.use_bias else None
        if not self.down:
            return ops.conv(x, self._weights(), self.kernel, self.weight.shape[0], mfma=False, bias=bias, res=res, out_scale=out_scale, out=out)
        kk, up, down, pad = fir_params('conv_down', self.resample_kernel, conv_k=self.kernel)
        folded = self._folded_weights if self._fold_taps is not None else None
        return padded_strided_conv(x, kk, pad, self._weights, self.kernel, self.weight.shape[0], bias, res, out_scale, out,
                                   layer=self.__dict__.get('_layer_name', 'Conv2d_0'), folded=folded)    # (its state_dict name: layerspp.bind_plan_scope)

    def forward(self, x):
        return self.run(View.from_nchw(x)).to_nchw()
