"""GPU: on-device global range, 8-bit quantisation and PSNR / SSIM / MAE (csrc/metrics.hip, mudiff_hip.metrics) against the host
path of the driver (driver.to_uint8, driver.psnr / ssim, driver.export_and_score) and the driver's --device_metrics end to end."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, REPO
from helpers import SMALL_CFGS
from mudiff_hip import MudiffHipError
from oracle import mudiff_oracle as O
from test_device_metrics_host import host_metrics, host_sums

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL_PSNR, TOL_SSIM, TOL_MAE = 1e-5, 1e-8, 1e-7


def _pairs(n, H, W, seed, noise=0.08):
    rng = np.random.default_rng(seed)
    gts = rng.uniform(-1, 1, (n, H, W)).astype(np.float32)
    preds = np.clip(gts + noise * rng.standard_normal(gts.shape), -1.3, 1.2).astype(np.float32)
    return preds, gts


def _u8_pairs(n, H, W, seed):
    rng = np.random.default_rng(seed)
    g8 = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    p8 = np.clip(g8.astype(np.int64) + rng.integers(-25, 26, (n, H, W)), 0, 255).astype(np.uint8)
    return p8, g8


# ---------------------------------------------------------------------------------------------------
def test_quantize_is_bit_exact_against_the_host():
    from mudiff_hip import driver, ops
    rng = np.random.default_rng(0)
    for H, W in ((7, 7), (37, 53), (240, 240), (256, 256)):
        x = rng.uniform(-1.5, 1.5, (3, H, W)).astype(np.float32)
        x[0, 0, :3] = [-0.9, 0.8, 0.0]
        for gmin, gmax in ((-1.0, 1.0), (-0.9, 0.8), (float(np.float32(-0.3)), float(np.float32(0.7)))):
            x[1, 1, :2] = [np.float32(gmin), np.float32(gmax)]        # values exactly at the ends of the range
            got = ops.quantize_u8(torch.from_numpy(x).to(DEV), gmin, gmax).cpu().numpy()
            assert np.array_equal(got, np.stack(driver.to_uint8(list(x), gmin, gmax))), (H, W, gmin, gmax)
        # a tiny range: nearly every value clips, the few inside land on all 256 levels
        lo = float(np.float32(0.25))
        hi = float(np.float32(lo + 1e-6))
        y = (lo + rng.uniform(-1e-6, 2e-6, (2, H, W))).astype(np.float32)
        got = ops.quantize_u8(torch.from_numpy(y).to(DEV), lo, hi).cpu().numpy()
        assert np.array_equal(got, np.stack(driver.to_uint8(list(y), lo, hi)))
    # the quantisation of every fp32 value in [-1, 1) on a fine grid, odd size (tails of the vector path)
    z = np.linspace(-1.2, 1.2, 1_000_003, dtype=np.float32)
    for gmin, gmax in ((-1.0, 1.0), (-0.7353, 0.9121)):
        got = ops.quantize_u8(torch.from_numpy(z).to(DEV), gmin, gmax).cpu().numpy()
        assert np.array_equal(got, driver.to_uint8([z], gmin, gmax)[0])
        got = ops.quantize_u8(torch.from_numpy(z).to(DEV)[1:], gmin, gmax).cpu().numpy()     # unaligned start: the scalar path
        assert np.array_equal(got, driver.to_uint8([z[1:]], gmin, gmax)[0])
    # a constant image: the (0, 1) fallback of export_and_score
    c = np.full((2, 9, 11), 0.3, np.float32)
    res = _score(c, c)
    assert (res['global_min'], res['global_max']) == (0.0, 1.0)
    assert np.array_equal(res['pred_u8'].cpu().numpy(), np.stack(driver.to_uint8(list(c), 0.0, 1.0)))
    with pytest.raises(ValueError):
        ops.quantize_u8(torch.from_numpy(c).to(DEV), 0.3, 0.3)


def test_value_range_matches_numpy():
    from mudiff_hip import ops
    rng = np.random.default_rng(1)
    for na, nb in ((1, 1), (7, 0), (1000, 333), (65537, 4099), (3 * 256 * 256 + 5, 2 * 240 * 240 + 1)):
        a = (rng.standard_normal(na) * 3).astype(np.float32)
        b = (rng.standard_normal(nb) * 3).astype(np.float32)
        ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        for x, y in ((ta, tb), (ta[1:], tb[1:]) if na > 1 and nb > 1 else (ta, tb)):
            got = ops.value_range(x, y).cpu().numpy()
            both = np.concatenate([x.cpu().numpy(), y.cpu().numpy()])
            assert got[0] == both.min() and got[1] == both.max(), (na, nb)
    empty = ops.value_range(torch.zeros(0, device=DEV), torch.zeros(0, device=DEV)).cpu().numpy()
    assert empty[0] == np.inf and empty[1] == -np.inf
    a = rng.standard_normal((4, 16, 16)).astype(np.float32)
    a[2, 5, 7] = np.nan
    assert np.isnan(ops.value_range(torch.from_numpy(a).to(DEV), torch.zeros(5, device=DEV)).cpu().numpy()).all()
    from mudiff_hip import metrics
    with pytest.raises(ValueError, match='NaN'):
        metrics.score_device(torch.from_numpy(a).to(DEV), torch.zeros(4, 16, 16, device=DEV))


# ---------------------------------------------------------------------------------------------------
def _score(preds, gts, **kw):
    from mudiff_hip import metrics
    return metrics.score_device(torch.from_numpy(preds).to(DEV), torch.from_numpy(gts).to(DEV), return_images=True, **kw)


@pytest.mark.parametrize('H,W', [(7, 7), (37, 53), (240, 240), (256, 256), (300, 517)])
def test_slice_metrics_against_the_host(H, W):
    """Per slice against driver.psnr / driver.ssim / the MAE of export_and_score on the same uint8 images, and against the fp64
    restatement from integer window sums (sse / sae exact)."""
    from mudiff_hip import ops
    p8, g8 = _u8_pairs(5 if H * W < 100_000 else 2, H, W, seed=H + W)
    p8[0] = g8[0]                                                     # identical images: PSNR inf
    sse, sae, ss = (t.cpu().numpy() for t in ops.slice_metrics_u8(torch.from_numpy(p8).to(DEV), torch.from_numpy(g8).to(DEV)))
    from mudiff_hip import metrics
    psnr, ssim, mae = metrics.per_slice_values(sse, sae, ss, H, W)
    for i in range(p8.shape[0]):
        e2, e1, s_ref = host_sums(p8[i], g8[i])
        assert (int(sse[i]), int(sae[i])) == (e2, e1)
        assert abs(ss[i] - s_ref) / ((H - 6) * (W - 6)) <= 1e-12
        hp, hs, hm = host_metrics(p8[i], g8[i])
        assert (psnr[i] == hp == float('inf')) if i == 0 else abs(psnr[i] - hp) <= TOL_PSNR
        assert abs(ssim[i] - hs) <= TOL_SSIM and abs(mae[i] - hm) <= TOL_MAE
    with pytest.raises(MudiffHipError, match='7x7'):
        ops.slice_metrics_u8(torch.zeros(1, 6, 9, dtype=torch.uint8, device=DEV), torch.zeros(1, 6, 9, dtype=torch.uint8, device=DEV))
    with pytest.raises(MudiffHipError, match='7x7'):
        ops.slice_metrics_u8(torch.zeros(1, 9, 6, dtype=torch.uint8, device=DEV), torch.zeros(1, 9, 6, dtype=torch.uint8, device=DEV))


def test_score_device_matches_export_and_score(tmp_path):
    from mudiff_hip import driver
    preds, gts = _pairs(6, 64, 80, seed=5)
    host = driver.export_and_score(list(preds), list(gts), str(tmp_path / 'host'))
    dev = _score(preds, gts, save_dir=str(tmp_path / 'dev'))
    assert dev['count'] == host['count'] == 6
    assert dev['global_min'] == host['global_min'] and dev['global_max'] == host['global_max']
    assert abs(dev['psnr'] - host['psnr']) <= TOL_PSNR and abs(dev['ssim'] - host['ssim']) <= TOL_SSIM and abs(dev['mae'] - host['mae']) <= TOL_MAE
    assert np.array_equal(dev['pred_u8'].cpu().numpy(), np.stack(driver.to_uint8(list(preds), host['global_min'], host['global_max'])))
    for sub in ('pred', 'gt'):
        names = sorted(os.listdir(tmp_path / 'host' / sub))
        assert names == sorted(os.listdir(tmp_path / 'dev' / sub)) and len(names) == 6
        for f in names:
            assert (tmp_path / 'host' / sub / f).read_bytes() == (tmp_path / 'dev' / sub / f).read_bytes(), f
    with pytest.raises(MudiffHipError, match='7x7'):
        _score(preds[:, :6, :], gts[:, :6, :])                        # H < 7


def test_identical_images_give_psnr_inf():
    preds, _ = _pairs(3, 16, 16, seed=6)
    res = _score(preds, preds.copy())
    assert res['psnr'] == float('inf') and res['mae'] == 0.0 and res['ssim'] == pytest.approx(1.0, abs=1e-12)


def test_deterministic_and_batch_independent():
    from mudiff_hip import ops
    p8, g8 = _u8_pairs(10, 256, 256, seed=7)
    tp, tg = torch.from_numpy(p8).to(DEV), torch.from_numpy(g8).to(DEV)
    a = [t.cpu().numpy() for t in ops.slice_metrics_u8(tp, tg)]
    b = [t.cpu().numpy() for t in ops.slice_metrics_u8(tp, tg)]
    s1 = [t.cpu().numpy() for t in ops.slice_metrics_u8(tp[:3], tg[:3])]
    s2 = [t.cpu().numpy() for t in ops.slice_metrics_u8(tp[3:], tg[3:])]
    for x, y, u, v in zip(a, b, s1, s2):
        assert x.tobytes() == y.tobytes()
        assert x.tobytes() == np.concatenate([u, v]).tobytes()


# ---------------------------------------------------------------------------------------------------
def _write_volumes(root, n, hw, seed):
    """As tests/test_driver.py builds them."""
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, 'test'), exist_ok=True)
    for mod in ('T1', 'T2', 'FLAIR', 'T1CE'):
        np.save(os.path.join(root, 'test', mod + '.npy'), (rng.standard_normal((n, hw, hw)) * 2).astype(np.float32))


def test_sampled_slices_score_alike_on_host_and_device(tmp_path):
    """The same sampled slices (one sample_slices run kept on the device) through both paths: identical PNGs, metrics within the
    tolerances.  Independent of run-to-run determinism of the sampler."""
    from mudiff_hip import driver, metrics
    from backbones.ncsnpp_generator_adagn_feat import NCSNpp, NCSNpp_adaptive
    _write_volumes(str(tmp_path), n=7, hw=32, seed=3)
    cfg = O.default_config(**SMALL_CFGS['s32'])
    g1, g2 = NCSNpp(cfg), NCSNpp_adaptive(cfg)
    g1.load_state_dict(O.make_state_dict(cfg, 'g1', 1234)); g2.load_state_dict(O.make_state_dict(cfg, 'g2', 1234))
    g1, g2 = g1.cuda().eval(), g2.cuda().eval()
    src = driver.SliceSource('test', str(tmp_path), 'T1CE')
    lo, preds, gts = driver.sample_slices(cfg, g1, g2, src, 4, torch.device(DEV), keep_on_device=True)
    assert lo == 0 and preds.is_cuda and gts.is_cuda and preds.shape == gts.shape == (7, 32, 32)
    host = driver.export_and_score(list(preds.cpu().numpy()), list(gts.cpu().numpy()), str(tmp_path / 'host'))
    dev = metrics.score_distributed(lo, preds, gts, str(tmp_path / 'dev'))
    assert (dev['count'], dev['global_min'], dev['global_max']) == (host['count'], host['global_min'], host['global_max'])
    assert abs(dev['psnr'] - host['psnr']) <= TOL_PSNR and abs(dev['ssim'] - host['ssim']) <= TOL_SSIM and abs(dev['mae'] - host['mae']) <= TOL_MAE
    for sub in ('pred', 'gt'):
        for f in sorted(os.listdir(tmp_path / 'host' / sub)):
            assert (tmp_path / 'host' / sub / f).read_bytes() == (tmp_path / 'dev' / sub / f).read_bytes(), f
    _, r1p, r1g = driver.sample_slices(cfg, g1, g2, src, 4, torch.device(DEV), rank=1, world=2, keep_on_device=True)
    assert r1p.shape == (3, 32, 32) and torch.equal(r1g, gts[4:])


_LOG = re.compile(r'Average PSNR: (\S+) dB  SSIM: (\S+)  MAE: (\S+) over (\d+) slices \(global range \[(\S+), (\S+)\]\)')


def test_driver_device_metrics_end_to_end(tmp_path):
    """`python -m mudiff_hip.driver` with and without --device_metrics on the same volumes (7 slices, batches of 4: the last one
    padded), deterministic sampling with the fixed seed: byte-identical PNGs, the same logged metrics."""
    data = tmp_path / 'data'
    _write_volumes(str(data), n=7, hw=32, seed=5)
    cfg = O.default_config(**SMALL_CFGS['s32'])
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.environ.get('PYTHONPATH', '')]), MUD_DETERMINISTIC='1')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    logs = {}
    for mode in ('host', 'device'):
        out = tmp_path / mode
        os.makedirs(out / 'exp7')
        for which, name in (('g1', 'gen_diffusive_1'), ('g2', 'gen_diffusive_2')):
            torch.save({'module.' + k: v for k, v in O.make_state_dict(cfg, which, 1234).items()}, out / 'exp7' / f'{name}.pth')
        cmd = [sys.executable, '-m', 'mudiff_hip.driver', '--input_path', str(data), '--output_path', str(out), '--exp', 'exp7',
               '--target_modality', 'T2', '--image_size', '32', '--num_channels_dae', '32', '--ch_mult', '1', '2', '4',
               '--attn_resolutions', '16', '--batch_size', '4'] + (['--device_metrics'] if mode == 'device' else [])
        p = subprocess.run(cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        m = _LOG.search(p.stderr)
        assert m, p.stderr[-2000:]
        logs[mode] = m.groups()
    h, d = logs['host'], logs['device']
    assert d[3] == h[3] == '7' and d[4:] == h[4:]
    for a, b in zip(h[:3], d[:3]):                                   # printed with 4 / 4 / 6 decimals
        assert abs(float(a) - float(b)) <= 10 ** -len(a.split('.')[1]), (h, d)
    for sub in ('pred', 'gt'):
        names = sorted(os.listdir(tmp_path / 'host' / 'generated_samples' / sub))
        assert names == sorted(os.listdir(tmp_path / 'device' / 'generated_samples' / sub)) and len(names) == 7
        for f in names:
            assert (tmp_path / 'host' / 'generated_samples' / sub / f).read_bytes() == \
                   (tmp_path / 'device' / 'generated_samples' / sub / f).read_bytes(), f


def test_metrics_cli(tmp_path):
    """`python -m mudiff_hip.metrics` on PNG directories (two image sizes, a file present on one side only, a batch size that splits
    the set) against the host restatement of tools/metric_calc.py."""
    from PIL import Image
    from mudiff_hip import metrics
    gt_dir, pred_dir = tmp_path / 'gt', tmp_path / 'pred'
    gt_dir.mkdir()
    pred_dir.mkdir()
    ref = []
    for i, (H, W) in enumerate([(40, 48)] * 4 + [(37, 53)] * 3):
        p8, g8 = _u8_pairs(1, H, W, seed=100 + i)
        Image.fromarray(g8[0]).save(gt_dir / f'img_{i:03d}.png')
        Image.fromarray(p8[0]).save(pred_dir / f'img_{i:03d}.png')
        ref.append(host_metrics(p8[0], g8[0]))
    Image.fromarray(np.zeros((8, 8), np.uint8)).save(gt_dir / 'only_gt.png')
    ps, ss, ma = (sum(r[k] for r in ref) / len(ref) for k in range(3))
    res = metrics.score_dirs(str(gt_dir), str(pred_dir), batch_size=3)
    assert res['count'] == 7
    assert abs(res['psnr'] - ps) <= TOL_PSNR and abs(res['ssim'] - ss) <= TOL_SSIM and abs(res['mae'] - ma) <= TOL_MAE
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.environ.get('PYTHONPATH', '')]))
    p = subprocess.run([sys.executable, '-m', 'mudiff_hip.metrics', '--gt_dir', str(gt_dir), '--pred_dir', str(pred_dir), '--batch_size', '3'],
                       cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.splitlines() == [f'Average PSNR: {res["psnr"]:.4f} dB', f'Average SSIM: {res["ssim"]:.4f}', f'Average MAE: {res["mae"]:.6f}']
