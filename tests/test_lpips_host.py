"""CPU: the host side of on-device LPIPS-alex (mudiff_hip.lpips_net, mudiff_hip.metrics with lpips) - the input table, the weight
loader's two layouts and its refusals, the merge of per-rank LPIPS values, the CLI flags and the C ABI declarations."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from lpips_ref import SCALE, SHIFT, seeded_weights, split_layout_b

LPIPS_SYMBOLS = ('mud_lpips_packed_bytes', 'mud_lpips_pack', 'mud_lpips_ws_bytes', 'mud_lpips_u8')


def test_input_table_is_torch_fp32_arithmetic_bit_for_bit():
    """All 256 x 3 entries against metric_calc's tensor path (numpy fp32 v / 255, torch x*2-1) and lpips's scaling layer in fp32."""
    from mudiff_hip.lpips_net import input_table
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    norm = np.array(v, dtype=np.float32) / 255.0
    t = torch.from_numpy(norm).unsqueeze(0).repeat(3, 1, 1).unsqueeze(0) * 2 - 1
    ref = (t - torch.Tensor([-.030, -.088, -.188])[None, :, None, None]) / torch.Tensor([.458, .448, .450])[None, :, None, None]
    tab = input_table()
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (3, 256)
    assert torch.equal(tab.view(torch.int32), ref.reshape(3, 256).contiguous().view(torch.int32))
    # given shift / scale (the optional scaling_layer keys) enter the same way
    sh, sc = torch.tensor([0.1, -0.2, 0.3]), torch.tensor([0.5, 0.25, 2.0])
    ref2 = (t - sh[None, :, None, None]) / sc[None, :, None, None]
    assert torch.equal(input_table(sh, sc).view(torch.int32), ref2.reshape(3, 256).contiguous().view(torch.int32))
    assert (SHIFT, SCALE) == ((-.030, -.088, -.188), (.458, .448, .450))


def test_loader_accepts_both_layouts(tmp_path):
    from mudiff_hip.lpips_net import LpipsAlex
    sd = seeded_weights(1)
    torch.save(sd, tmp_path / 'full.pth')
    alex, lin = split_layout_b(sd)
    torch.save(alex, tmp_path / 'alexnet.pth')
    torch.save(lin, tmp_path / 'alex.pth')
    a = LpipsAlex.from_files(str(tmp_path / 'full.pth'))
    b = LpipsAlex.from_files(str(tmp_path / 'alexnet.pth'), lin=str(tmp_path / 'alex.pth'))
    c = LpipsAlex.from_state_dict({'module.' + k: v for k, v in sd.items()})          # a DataParallel prefix is dropped
    for x in (b, c):
        for u, v in zip(a.conv_w + a.conv_b + a.lin_w, x.conv_w + x.conv_b + x.lin_w):
            assert torch.equal(u, v)
        assert torch.equal(a.table, x.table)
    assert [tuple(w.shape) for w in a.lin_w] == [(64,), (192,), (384,), (256,), (256,)]
    assert a.packed is None                                                          # nothing on a device until .to()
    # scaling_layer keys in a full lpips state dict are used
    sd2 = dict(sd)
    sd2['scaling_layer.shift'] = torch.tensor([0.1, 0.2, 0.3]).view(1, 3, 1, 1)
    sd2['scaling_layer.scale'] = torch.tensor([0.5, 0.5, 0.5]).view(1, 3, 1, 1)
    d = LpipsAlex.from_state_dict(sd2)
    assert d.table[0, 0].item() == pytest.approx((-1 - 0.1) / 0.5)


def test_loader_refuses_a_missing_key_and_a_wrong_shape(tmp_path):
    from mudiff_hip.lpips_net import LpipsAlex
    sd = seeded_weights(2)
    for key in ('net.slice3.6.weight', 'net.slice5.10.bias', 'lin4.model.1.weight'):
        bad = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(ValueError, match=re.escape(key)):
            LpipsAlex.from_state_dict(bad)
    bad = dict(sd)
    bad['net.slice2.3.weight'] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=re.escape('net.slice2.3.weight')):
        LpipsAlex.from_state_dict(bad)
    bad = dict(sd)
    bad['lin1.model.1.weight'] = torch.zeros(1, 191, 1, 1)
    with pytest.raises(ValueError, match='lin1.model.1.weight'):
        LpipsAlex.from_state_dict(bad)
    alex, lin = split_layout_b(sd)
    torch.save(alex, tmp_path / 'alexnet.pth')
    with pytest.raises(ValueError, match='lin0.model.1.weight'):                   # (b) without its lin file
        LpipsAlex.from_files(str(tmp_path / 'alexnet.pth'))


# ---------------------------------------------------------------------------------------------------
def _parts(n=10, H=32, W=40, seed=0):
    rng = np.random.default_rng(seed)
    sse = rng.integers(1, 255 * 255 * H * W // 50, n).astype(np.int64)
    sae = rng.integers(0, 255 * H * W // 20, n).astype(np.int64)
    ss = rng.uniform(0.2, 1.0, n) * (H - 6) * (W - 6)
    lp = rng.uniform(0.0, 0.7, n)
    return sse, sae, ss, lp


def test_combine_shards_with_lpips():
    from mudiff_hip import metrics
    sse, sae, ss, lp = _parts()
    part = lambda lo, hi, with_lp=True: dict(lo=lo, sse=sse[lo:hi], sae=sae[lo:hi], ssim_sum=ss[lo:hi], H=32, W=40,  # noqa: E731
                                             **(dict(lpips=lp[lo:hi]) if with_lp else {}))
    one = metrics.combine_shards([part(0, 10)])
    acc = 0.0
    for v in lp:
        acc += float(v)
    assert one['lpips'] == acc / 10 and np.array_equal(one['lpips_per_slice'], lp)
    plain = metrics.combine_shards([part(0, 10, False)])
    assert 'lpips' not in plain and 'lpips_per_slice' not in plain
    assert {k for k in one} - {k for k in plain} == {'lpips', 'lpips_per_slice'}
    for k in plain:
        assert np.array_equal(np.asarray(plain[k]), np.asarray(one[k])), k
    for parts in ([part(3, 7), part(7, 7), part(0, 3), part(7, 10)], [part(7, 10), part(0, 7)],
                  [part(0, 0), part(0, 10), part(10, 10)], [part(0, 0, False), part(0, 10), part(10, 10, False)]):
        got = metrics.combine_shards(parts)
        assert got['lpips'] == one['lpips'] and np.array_equal(got['lpips_per_slice'], one['lpips_per_slice'])
    with pytest.raises(ValueError, match='LPIPS'):
        metrics.combine_shards([part(0, 4), part(4, 10, False)])
    with pytest.raises(ValueError, match='LPIPS'):
        metrics.combine_shards([dict(part(0, 4), lpips=lp[:3]), part(4, 10)])


def test_lpips_totals_add_the_taps_in_order():
    from mudiff_hip.lpips_net import lpips_totals
    d = np.random.default_rng(4).uniform(0, 0.3, (7, 5))
    got = lpips_totals(d)
    for i in range(7):
        assert got[i] == (((d[i, 0] + d[i, 1]) + d[i, 2]) + d[i, 3]) + d[i, 4]


# ---------------------------------------------------------------------------------------------------
def test_metrics_cli_lpips_flags():
    from mudiff_hip import metrics
    base = ['--gt_dir', 'g', '--pred_dir', 'p']
    a = metrics.parse_args(base)
    assert a.lpips_weights is None and a.lpips_lin is None
    a = metrics.parse_args(base + ['--lpips_weights', 'w.pth', '--lpips_lin', 'l.pth'])
    assert (a.lpips_weights, a.lpips_lin) == ('w.pth', 'l.pth')
    assert metrics.load_lpips(metrics.parse_args(base)) is None
    with pytest.raises(SystemExit):
        metrics.parse_args(base + ['--lpips_lin', 'l.pth'])


def test_driver_lpips_flags_need_device_metrics():
    from mudiff_hip import driver
    a = driver.parse_args([])
    assert a.lpips_weights is None and a.device_metrics is False
    a = driver.parse_args(['--device_metrics', '--lpips_weights', 'w.pth'])
    assert a.lpips_weights == 'w.pth' and a.lpips_lin is None
    a = driver.parse_args(['--device_metrics', '--lpips_weights', 'w.pth', '--lpips_lin', 'l.pth'])
    assert a.lpips_lin == 'l.pth'
    with pytest.raises(SystemExit):
        driver.parse_args(['--lpips_weights', 'w.pth'])                           # the host path has no LPIPS
    with pytest.raises(SystemExit):
        driver.parse_args(['--device_metrics', '--lpips_lin', 'l.pth'])


# ---------------------------------------------------------------------------------------------------
def test_lpips_symbols_are_declared_and_bound():
    import mudiff_hip
    txt = open(os.path.join(REPO, 'include', 'mudiff_hip.h')).read()
    for name in LPIPS_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', txt), name
        assert name in mudiff_hip._SIGNATURES, name
    lib = mudiff_hip.load()
    assert lib.mud_version() >= 113
    assert lib.mud_lpips_packed_bytes() > 4 * (384 * 64 + 1600 * 192 + 1728 * 384 + 3456 * 256 + 2304 * 256)
    assert lib.mud_lpips_packed_bytes() % 256 == 0
    assert lib.mud_lpips_ws_bytes(1, 256, 256) > 0 and lib.mud_lpips_ws_bytes(0, 31, 31) == 0
    for n, H, W in ((1, 30, 64), (1, 64, 30), (-1, 64, 64)):
        assert lib.mud_lpips_ws_bytes(n, H, W) == -1
    # linear in n up to alignment: a chunk of k slices never needs more than k single-slice workspaces
    one = lib.mud_lpips_ws_bytes(1, 256, 256)
    for k in (2, 7, 200):
        assert lib.mud_lpips_ws_bytes(k, 256, 256) <= k * one


def test_lpips_refuses_bad_arguments_before_any_launch():
    """Argument checks come before the first launch, so they run without a GPU: every refusal returns MUD_ERR_ARG."""
    import ctypes as C
    import mudiff_hip
    lib = mudiff_hip.load()
    fake = 1 << 20                                            # never dereferenced: the call is refused first
    ws = lib.mud_lpips_ws_bytes(2, 64, 64)
    cases = [
        ((0, fake, 2, 64, 64, fake, fake, fake, ws), 'null'),
        ((fake, fake, 2, 30, 64, fake, fake, fake, ws), '31'),
        ((fake, fake, 2, 64, 30, fake, fake, fake, ws), '31'),
        ((fake, fake, -1, 64, 64, fake, fake, fake, ws), '31'),
        ((fake, fake, 2, 64, 64, fake, fake, fake, ws - 1), 'ws holds'),
        ((fake, fake, 2, 64, 64, fake + 4, fake, fake, ws), 'aligned'),
        ((fake, fake, 2, 64, 64, fake, fake + 4, fake, ws), 'aligned'),
        ((fake, fake, 2, 64, 64, fake, fake, fake + 8, ws), 'aligned'),
    ]
    for (p, g, n, H, W, packed, out, w, nb), msg in cases:
        code = lib.mud_lpips_u8(C.c_void_p(p), C.c_void_p(g), n, H, W, C.c_void_p(packed), C.c_void_p(out), C.c_void_p(w), nb, None)
        assert code == 1, (n, H, W, msg)
        assert msg in lib.mud_last_error().decode(), (msg, lib.mud_last_error())
    arr = (C.c_void_p * 5)(*([fake] * 5))
    assert lib.mud_lpips_pack(None, arr, arr, arr, C.c_void_p(fake), None) == 1
    assert lib.mud_lpips_pack(C.c_void_p(fake), arr, arr, arr, C.c_void_p(fake + 4), None) == 1
    assert 'aligned' in lib.mud_last_error().decode()
    arr2 = (C.c_void_p * 5)(fake, fake, None, fake, fake)
    assert lib.mud_lpips_pack(C.c_void_p(fake), arr, arr2, arr, C.c_void_p(fake), None) == 1
    assert 'layer 3' in lib.mud_last_error().decode()
