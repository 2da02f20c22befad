"""fp64 restatement of LPIPS-alex (lpips v0.1, net='alex', eval) on uint8 grayscale pairs, written from the definition with
torch-CPU float64 F.conv2d / F.max_pool2d, and seeded weights in both accepted file layouts.  Test helper, not a test module."""
import numpy as np
import torch
import torch.nn.functional as F

CONVS = ((64, 3, 11, 11, 4, 2), (192, 64, 5, 5, 1, 2), (384, 192, 3, 3, 1, 1), (256, 384, 3, 3, 1, 1), (256, 256, 3, 3, 1, 1))
CONV_INDEX = (0, 3, 6, 8, 10)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def seeded_weights(seed, scale=1.0, bias=0.0, last_bias=None, last_scale=1.0):
    """A layout-(a) state dict: He-scaled normal conv weights times `scale`, biases uniform(-0.1, 0.1) + `bias` (conv5: weights also
    times `last_scale`, biases + `last_bias` if given), lin weights uniform [0, 0.2) - the sign lpips's trained lin layers have."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, ((co, ci, kh, kw, _, _), idx) in enumerate(zip(CONVS, CONV_INDEX)):
        std = (2.0 / (ci * kh * kw)) ** 0.5 * scale * (last_scale if i == 4 else 1.0)
        sd[f'net.slice{i + 1}.{idx}.weight'] = torch.randn(co, ci, kh, kw, generator=g) * std
        b = (torch.rand(co, generator=g) - 0.5) * 0.2 + bias
        if i == 4 and last_bias is not None:
            b = b + last_bias
        sd[f'net.slice{i + 1}.{idx}.bias'] = b
    for i, (co, *_rest) in enumerate(CONVS):
        sd[f'lin{i}.model.1.weight'] = torch.rand(1, co, 1, 1, generator=g) * 0.2
    return sd


def split_layout_b(sd):
    """The same weights as (torchvision AlexNet state dict with a classifier, lpips lin file)."""
    alex, lin = {}, {}
    for i, idx in enumerate(CONV_INDEX):
        alex[f'features.{idx}.weight'] = sd[f'net.slice{i + 1}.{idx}.weight'].clone()
        alex[f'features.{idx}.bias'] = sd[f'net.slice{i + 1}.{idx}.bias'].clone()
    alex['classifier.1.weight'] = torch.zeros(4, 9216)
    alex['classifier.1.bias'] = torch.zeros(4)
    for i in range(5):
        lin[f'lin{i}.model.1.weight'] = sd[f'lin{i}.model.1.weight'].clone()
    return alex, lin


def _input(u8, shift, scale):
    """metric_calc + lpips's scaling layer: fp32 v/255, *2-1, (x - shift) / scale, all in fp32 -> fp64 [n, 3, H, W]."""
    x = torch.from_numpy(np.asarray(u8, np.float32) / np.float32(255.0))[:, None].repeat(1, 3, 1, 1) * 2 - 1
    x = (x - torch.tensor(shift, dtype=torch.float32).view(1, 3, 1, 1)) / torch.tensor(scale, dtype=torch.float32).view(1, 3, 1, 1)
    return x.double()


def features(u8, sd, shift=SHIFT, scale=SCALE):
    """The 5 taps relu1..relu5 (fp64 NCHW) of uint8 images [n, H, W]."""
    x = _input(u8, shift, scale)
    taps = []
    for i, ((_, _, _, _, stride, pad), idx) in enumerate(zip(CONVS, CONV_INDEX)):
        if i in (1, 2):
            x = F.max_pool2d(x, 3, 2)
        w = sd[f'net.slice{i + 1}.{idx}.weight'].double()
        b = sd[f'net.slice{i + 1}.{idx}.bias'].double()
        x = F.relu(F.conv2d(x, w, b, stride=stride, padding=pad))
        taps.append(x)
    return taps


def lpips_taps(pred_u8, gt_u8, sd, return_features=False):
    """fp64 [n, 5]: d_l = mean over pixels of sum_c lin_l[c] (f0/(|f0| + 1e-10) - f1/(|f1| + 1e-10))^2 per tap."""
    with torch.no_grad():
        f0, f1 = features(pred_u8, sd), features(gt_u8, sd)
        out = []
        for i, (a, b) in enumerate(zip(f0, f1)):
            na = a / (torch.sqrt((a * a).sum(1, keepdim=True)) + 1e-10)
            nb = b / (torch.sqrt((b * b).sum(1, keepdim=True)) + 1e-10)
            w = sd[f'lin{i}.model.1.weight'].double().view(1, -1, 1, 1)
            out.append((w * (na - nb) ** 2).sum(1).mean((1, 2)))
        res = torch.stack(out, 1).numpy()
    return (res, f0, f1) if return_features else res
