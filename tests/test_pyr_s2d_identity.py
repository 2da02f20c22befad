"""The identity behind the input pyramid's folded down-sampler, in fp64 on the CPU: a separable 4x4 FIR padded
(2, 2) followed by a 3x3 stride-2 pad-0 convolution W is ONE 3x3 stride-1 pad-1 convolution over the 2x2 space-to-depth view of the
input, with the weights backbones/up_or_down_sampling.fold_fir_conv_weight composes and in the channel order ops.s2d_fold /
mud_conv_args.in_s2d use.  Pins the tap flip (upfirdn2d correlates with the flipped kernel) and the zero padding."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

torch.set_grad_enabled(False)


def _fir_then_conv(x, w, k1d):
    """conv_downsample_2d as the reference computes it: zero-pad (2, 2), correlate with the FLIPPED 4x4 kernel, conv3x3 stride 2."""
    B, Cc, H, W = x.shape
    k2 = torch.from_numpy(np.outer(k1d, k1d)).double().flip(0, 1)[None, None]
    xf = F.conv2d(F.pad(x, (2, 2, 2, 2)).reshape(B * Cc, 1, H + 4, W + 4), k2).reshape(B, Cc, H + 1, W + 1)
    return F.conv2d(xf, w, stride=2)


def _folded(x, w, k1d):
    from backbones.up_or_down_sampling import fold_fir_conv_weight
    from mudiff_hip import ops
    xv = ops.s2d_fold(x.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)           # NHWC fold, back to NCHW for F.conv2d
    return F.conv2d(xv, fold_fir_conv_weight(w, k1d, dtype=torch.float64), padding=1)


# tiles of the 3x3 kernel are 32 view columns x 4 / 8 view rows: one tile, odd and even tile counts along both axes, ragged sizes, and
# images so small that every output touches a border
@pytest.mark.parametrize('H,W', [(2, 2), (4, 6), (16, 64), (24, 80), (48, 128), (40, 192), (6, 130)])
@pytest.mark.parametrize('taps', [(1, 3, 3, 1), (1, 2, 5, -3)], ids=['symmetric', 'asymmetric'])
def test_fir_then_stride2_conv_is_one_conv_on_the_folded_view(H, W, taps):
    gen = torch.Generator().manual_seed(H * 1000 + W)
    B, Cin, Cout = 2, 3, 5
    k1d = np.asarray(taps, dtype=np.float64) / np.sum(taps)
    x = torch.randn(B, Cin, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen, dtype=torch.float64)
    ref, got = _fir_then_conv(x, w, k1d), _folded(x, w, k1d)
    assert got.shape == ref.shape == (B, Cout, H // 2, W // 2)
    err = float((got - ref).abs().max()) / float(ref.abs().max())
    assert err <= 1e-12, err
    # the borders alone: an input that lives only on the outermost ring of pixels
    ring = torch.zeros_like(x)
    ring[:, :, 0], ring[:, :, -1], ring[:, :, :, 0], ring[:, :, :, -1] = x[:, :, 0], x[:, :, -1], x[:, :, :, 0], x[:, :, :, -1]
    ref, got = _fir_then_conv(ring, w, k1d), _folded(ring, w, k1d)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_the_model_filter_is_the_separable_one_the_fold_takes():
    """fir_params('conv_down') of the model's (1, 3, 3, 1) kernel: pad (2, 2), exactly t (x) t with t = (1, 3, 3, 1) / 8; a filter that is
    not separable, or another padding, is turned down (the layer then keeps its two launches)."""
    from backbones.up_or_down_sampling import fir_params, separable_taps
    kk, up, down, pad = fir_params('conv_down', (1, 3, 3, 1), conv_k=3)
    assert (up, down, tuple(pad)) == (1, 1, (2, 2))
    t = separable_taps(kk, pad)
    assert t is not None and np.array_equal(t, np.array([1, 3, 3, 1]) / 8.0)
    assert separable_taps(kk, (2, 1)) is None
    assert separable_taps(np.ones((1, 1), np.float32), (0, 1)) is None
    bad = np.array(kk, dtype=np.float64)
    bad[0, 0] *= 2
    assert separable_taps(bad, pad) is None


def test_the_fold_is_rounded_to_fp32_once():
    from backbones.up_or_down_sampling import fold_fir_conv_weight
    gen = torch.Generator().manual_seed(9)
    w = torch.randn(8, 16, 3, 3, generator=gen) / 12.0
    t = np.array([1, 3, 3, 1]) / 8.0
    w32, w64 = fold_fir_conv_weight(w, t), fold_fir_conv_weight(w, t, dtype=torch.float64)
    assert w32.dtype == torch.float32 and w32.shape == (8, 64, 3, 3) and torch.equal(w32, w64.float())
