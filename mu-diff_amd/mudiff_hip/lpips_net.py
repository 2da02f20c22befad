"""LPIPS with the AlexNet backbone (lpips v0.1, net='alex', defaults, eval mode) - the fourth number of the reference's
tools/metric_calc.py - on the device (csrc/lpips.hip through mudiff_hip.ops.lpips_u8).

The weights are not shipped: users bring the files, as they bring their generator checkpoints.  Two layouts are accepted:

(a) one saved `lpips.LPIPS(net='alex').state_dict()`: net.slice1.0.*, net.slice2.3.*, net.slice3.6.*, net.slice4.8.*, net.slice5.10.*
    (weight and bias), lin{0..4}.model.1.weight and optionally scaling_layer.shift / scaling_layer.scale;
(b) a torchvision AlexNet state dict (features.{0,3,6,8,10}.*; classifier.* is ignored) plus lpips's weights/v0.1/alex.pth (the
    lin{0..4}.model.1.weight keys).

    net = LpipsAlex.from_files('alex_lpips_full.pth').to('cuda:0')                    # (a)
    net = LpipsAlex.from_files('alexnet-owt.pth', lin='weights/v0.1/alex.pth').to(dev)  # (b)
    taps = mudiff_hip.ops.lpips_u8(pred_u8, gt_u8, net)                                 # fp64 [n, 5]; LPIPS = row sum

The grayscale input path is metric_calc's: a uint8 'L' pixel v becomes x = (float32(v) / 255) * 2 - 1, repeated to 3 channels, and
lpips's scaling layer computes (x - shift_c) / scale_c.  All 256 x 3 inputs are tabulated here with that fp32 arithmetic."""
from __future__ import annotations

import numpy as np
import torch

# lpips.pretrained_networks.ScalingLayer (v0.1)
DEFAULT_SHIFT = (-.030, -.088, -.188)
DEFAULT_SCALE = (.458, .448, .450)

# torchvision alexnet().features indices of the 5 convs, the lpips slice that holds each, and their shapes
CONV_INDEX = (0, 3, 6, 8, 10)
CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))
CHANNELS = tuple(s[0] for s in CONV_SHAPES)


def input_table(shift=None, scale=None):
    """fp32 [3, 256]: the scaled network input of gray level v in channel c, computed as metric_calc + lpips compute it
    (numpy fp32 v / 255.0, then torch fp32 x * 2 - 1, (x - shift) / scale)."""
    shift = torch.tensor(DEFAULT_SHIFT, dtype=torch.float32) if shift is None else torch.as_tensor(shift, dtype=torch.float32).reshape(3)
    scale = torch.tensor(DEFAULT_SCALE, dtype=torch.float32) if scale is None else torch.as_tensor(scale, dtype=torch.float32).reshape(3)
    norm = torch.from_numpy(np.arange(256, dtype=np.float32) / 255.0)
    x = norm.reshape(1, 1, 1, 256).repeat(1, 3, 1, 1) * 2 - 1
    return ((x - shift.reshape(1, 3, 1, 1)) / scale.reshape(1, 3, 1, 1)).reshape(3, 256).contiguous()


def _get(sd, key, shape):
    if key not in sd:
        raise ValueError(f'LPIPS weights: missing key {key!r}')
    t = sd[key]
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f'LPIPS weights: {key!r} has shape {got}, expected {tuple(shape)}')
    return t.detach().to('cpu', torch.float32).contiguous()


class LpipsAlex:
    """The weights of lpips.LPIPS(net='alex') on the host; .to(device) packs them for the kernels (`packed`, `device`)."""

    def __init__(self, conv_w, conv_b, lin_w, shift=None, scale=None):
        self.conv_w, self.conv_b, self.lin_w = list(conv_w), list(conv_b), list(lin_w)
        self.shift, self.scale = shift, scale
        self.table = input_table(shift, scale)
        self.packed, self.device = None, None

    @classmethod
    def from_state_dict(cls, sd):
        """From layout (a), or from the keys of layout (b) merged into one dict.  Missing keys and wrong shapes raise ValueError."""
        sd = {k[len('module.'):] if k.startswith('module.') else k: v for k, v in sd.items()}
        full = any(k.startswith('net.slice') for k in sd)
        conv_w, conv_b = [], []
        for i, (idx, shape) in enumerate(zip(CONV_INDEX, CONV_SHAPES)):
            pre = f'net.slice{i + 1}.{idx}.' if full else f'features.{idx}.'
            conv_w.append(_get(sd, pre + 'weight', shape))
            conv_b.append(_get(sd, pre + 'bias', shape[:1]))
        lin_w = [_get(sd, f'lin{i}.model.1.weight', (1, c, 1, 1)).reshape(c) for i, c in enumerate(CHANNELS)]
        shift = _get(sd, 'scaling_layer.shift', (1, 3, 1, 1)).reshape(3) if 'scaling_layer.shift' in sd else None
        scale = _get(sd, 'scaling_layer.scale', (1, 3, 1, 1)).reshape(3) if 'scaling_layer.scale' in sd else None
        return cls(conv_w, conv_b, lin_w, shift, scale)

    @classmethod
    def from_files(cls, weights, lin=None):
        """`weights`: a saved lpips.LPIPS(net='alex') state dict (a), or a torchvision AlexNet state dict (b) with `lin` =
        lpips's weights/v0.1/alex.pth.  Read with torch.load(map_location='cpu', weights_only=True)."""
        sd = dict(torch.load(weights, map_location='cpu', weights_only=True))
        if lin is not None:
            sd.update(torch.load(lin, map_location='cpu', weights_only=True))
        return cls.from_state_dict(sd)

    def to(self, device):
        """Pack the weights on `device` (a no-op if they already are) -> self."""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if self.packed is not None and self.device == device:
            return self
        from . import ops
        dev = lambda ts: [t.to(device) for t in ts]        # noqa: E731
        self.packed = ops.lpips_pack(self.table.reshape(-1).to(device), dev(self.conv_w), dev(self.conv_b), dev(self.lin_w))
        self.device = device
        return self


def lpips_totals(taps):
    """Per-slice LPIPS from the per-tap values [n, 5] (any array-like) -> fp64 numpy [n], added in tap order."""
    d = np.asarray(taps, np.float64).reshape(-1, 5)
    return (((d[:, 0] + d[:, 1]) + d[:, 2]) + d[:, 3]) + d[:, 4]
