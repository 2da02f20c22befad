"""GPU: LPIPS-alex on the device (csrc/lpips.hip, ops.lpips_u8, metrics with lpips=, the driver's --lpips_weights) against the fp64
restatement in tests/lpips_ref.py, plus its exactness guarantees (identical images, batch / chunk / run independence)."""
import ctypes as C
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import PKG, REPO
from helpers import SMALL_CFGS
from lpips_ref import lpips_taps, seeded_weights, split_layout_b
from oracle import mudiff_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ABS, REL = 2e-6, 1e-5

# weight sets: (seed, scale, bias, conv5 bias, conv5 weight scale).  The last one drives conv5's biases negative against small
# weights, so whole relu5 pixels are zero (all of them below ~64x64, about 30 % at 240x240) and the head's 1e-10 guard decides them.
WEIGHTS = {'unit': (11, 1.0, 0.0, None, 1.0), 'small': (12, 0.35, 0.02, None, 1.0), 'large': (13, 2.5, -0.05, None, 1.0),
           'dead5': (14, 1.0, 0.0, -1.2, 0.1)}


def _net(kind):
    from mudiff_hip.lpips_net import LpipsAlex
    sd = seeded_weights(*WEIGHTS[kind])
    return sd, LpipsAlex.from_state_dict(sd).to(DEV)


def _u8_pairs(n, H, W, seed, amp=40):
    """Smooth-ish images (a blurred field plus noise) and predictions that differ by bounded noise."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0, 255, (n, H // 4 + 2, W // 4 + 2))
    base = np.kron(base, np.ones((4, 4)))[:, :H, :W]
    g8 = np.clip(base + rng.normal(0, 20, (n, H, W)), 0, 255).astype(np.uint8)
    p8 = np.clip(g8.astype(np.int64) + rng.integers(-amp, amp + 1, (n, H, W)), 0, 255).astype(np.uint8)
    return p8, g8


def _dev(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in a]


def _check(got, ref, what):
    err = np.abs(got - ref)
    bound = ABS + REL * np.abs(ref)
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    assert (err <= bound).all(), f'{what}: worst |delta| {err[worst]:.3e} at (slice, tap) {worst}, ref {ref[worst]:.6e}'


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['unit', 'small', 'large', 'dead5'])
@pytest.mark.parametrize('H,W', [(31, 31), (37, 53), (240, 240), (256, 256)])
def test_taps_match_the_fp64_restatement(H, W, kind):
    from mudiff_hip import ops
    sd, net = _net(kind)
    n = 4 if H * W < 10_000 else 2
    p8, g8 = _u8_pairs(n, H, W, seed=H * 7 + W + len(kind))
    got = ops.lpips_u8(*_dev(p8, g8), net)
    assert got.dtype == torch.float64 and tuple(got.shape) == (n, 5) and got.is_cuda
    ref, f0, f1 = lpips_taps(p8, g8, sd, return_features=True)
    _check(got.cpu().numpy(), ref, f'{H}x{W} {kind}')
    assert (ref[:, :4] > 0).all()
    if kind == 'dead5':                                        # the case this weight set is for: all-zero relu5 pixels
        dead = ((f0[4] == 0).all(1) | (f1[4] == 0).all(1)).sum().item()
        assert dead > 0, 'no all-zero relu5 pixel: the 1e-10 guard is not exercised'


def test_identical_images_give_exactly_zero():
    from mudiff_hip import ops
    for kind in ('unit', 'dead5'):
        _, net = _net(kind)
        p8, g8 = _u8_pairs(3, 64, 72, seed=3)
        a, b = _dev(g8, g8.copy())
        got = ops.lpips_u8(a, b, net).cpu().numpy()
        assert (got == 0.0).all(), got
        mixed = np.concatenate([p8[:1], g8[1:2], p8[2:]])     # one identical pair inside a batch of different ones
        got = ops.lpips_u8(*_dev(mixed, g8), net).cpu().numpy()
        assert (got[1] == 0.0).all() and (got[[0, 2], :4] > 0).all()


def test_batch_run_and_chunk_independence():
    from mudiff_hip import ops
    _, net = _net('unit')
    p8, g8 = _u8_pairs(7, 96, 80, seed=5)
    tp, tg = _dev(p8, g8)
    whole = ops.lpips_u8(tp, tg, net)
    assert torch.equal(whole, ops.lpips_u8(tp, tg, net))                       # two runs
    singles = torch.cat([ops.lpips_u8(tp[i:i + 1], tg[i:i + 1], net) for i in range(7)])
    assert torch.equal(whole, singles)                                          # batch vs one at a time
    lib_ws = __import__('mudiff_hip').load().mud_lpips_ws_bytes
    cap = lib_ws(3, 96, 80)                                                     # chunks of 3: 3 + 3 + 1
    chunked = ops.lpips_u8(tp, tg, net, max_ws_bytes=cap)
    assert torch.equal(whole, chunked)
    parts = torch.cat([ops.lpips_u8(tp[:2], tg[:2], net), ops.lpips_u8(tp[2:], tg[2:], net)])
    assert torch.equal(chunked, parts)
    assert ops.lpips_u8(tp[:0], tg[:0], net).shape == (0, 5)


def test_raw_entry_points_refuse_bad_arguments_without_a_launch():
    import mudiff_hip
    from mudiff_hip import ops
    lib = mudiff_hip.load()
    _, net = _net('unit')
    p8, g8 = _dev(*_u8_pairs(2, 64, 64, seed=6))
    ws_n = lib.mud_lpips_ws_bytes(2, 64, 64)
    ws = torch.empty(ws_n + 64, dtype=torch.uint8, device=DEV)
    out = torch.full((2 * 5 + 2,), 7.0, dtype=torch.float64, device=DEV)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)                        # noqa: E731
    good = [P(p8), P(g8), 2, 64, 64, P(net.packed), P(out), P(ws), ws_n, None]
    cases = {0: None, 1: None, 5: None, 6: None, 7: None}                       # null pointers
    bad = [dict({i: v}) for i, v in cases.items()]
    bad += [{3: 30}, {4: 17}, {2: -1}, {8: ws_n - 1}, {5: P(net.packed, 4)}, {7: P(ws, 8)}, {6: P(out, 4)}]
    for change in bad:
        args = list(good)
        for i, v in change.items():
            args[i] = v
        assert lib.mud_lpips_u8(*args) == 1, change
        assert lib.mud_last_error(), change
    torch.cuda.synchronize()
    assert (out.cpu() == 7.0).all(), 'a refused call wrote its output'
    assert lib.mud_lpips_u8(*good) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:10].view(2, 5), ops.lpips_u8(p8, g8, net))
    with pytest.raises(mudiff_hip.MudiffHipError, match='31x31'):
        ops.lpips_u8(*_dev(np.zeros((1, 30, 40), np.uint8), np.zeros((1, 30, 40), np.uint8)), net)


# ---------------------------------------------------------------------------------------------------
def test_score_dirs_with_lpips(tmp_path):
    """PNG directories, two image sizes, a batch size that splits the set: LPIPS per slice against the restatement, PSNR / SSIM /
    MAE bit-identical to the call without LPIPS, and the CLI's fourth line."""
    from PIL import Image
    from mudiff_hip import metrics
    from mudiff_hip.lpips_net import LpipsAlex
    sd, _ = _net('unit')
    alex, lin = split_layout_b(sd)
    torch.save(alex, tmp_path / 'alexnet.pth')
    torch.save(lin, tmp_path / 'alex.pth')
    net = LpipsAlex.from_files(str(tmp_path / 'alexnet.pth'), lin=str(tmp_path / 'alex.pth'))
    gt_dir, pred_dir = tmp_path / 'gt', tmp_path / 'pred'
    gt_dir.mkdir()
    pred_dir.mkdir()
    ref = []
    for i, (H, W) in enumerate([(48, 40)] * 4 + [(37, 53)] * 3):
        p8, g8 = _u8_pairs(1, H, W, seed=200 + i)
        Image.fromarray(g8[0]).save(gt_dir / f'img_{i:03d}.png')
        Image.fromarray(p8[0]).save(pred_dir / f'img_{i:03d}.png')
        ref.append(lpips_taps(p8, g8, sd)[0])
    ref = np.array(ref)
    plain = metrics.score_dirs(str(gt_dir), str(pred_dir), batch_size=3)
    res = metrics.score_dirs(str(gt_dir), str(pred_dir), batch_size=3, lpips=net)
    assert 'lpips' not in plain and res['count'] == 7
    for k in plain:
        assert np.array_equal(np.asarray(plain[k]), np.asarray(res[k])), k
    tol = (ABS + REL * np.abs(ref)).sum(1)
    assert (np.abs(res['lpips_per_slice'] - ref.sum(1)) <= tol).all(), (res['lpips_per_slice'], ref.sum(1))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.environ.get('PYTHONPATH', '')]))
    base = [sys.executable, '-m', 'mudiff_hip.metrics', '--gt_dir', str(gt_dir), '--pred_dir', str(pred_dir), '--batch_size', '3']
    p = subprocess.run(base + ['--lpips_weights', str(tmp_path / 'alexnet.pth'), '--lpips_lin', str(tmp_path / 'alex.pth')], cwd=REPO,
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.splitlines() == [f'Average PSNR: {res["psnr"]:.4f} dB', f'Average SSIM: {res["ssim"]:.4f}', f'Average MAE: {res["mae"]:.6f}',
                                     f'Average LPIPS: {res["lpips"]:.6f}']


# ---------------------------------------------------------------------------------------------------
def _write_volumes(root, n, hw, seed):
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, 'test'), exist_ok=True)
    for mod in ('T1', 'T2', 'FLAIR', 'T1CE'):
        np.save(os.path.join(root, 'test', mod + '.npy'), (rng.standard_normal((n, hw, hw)) * 2).astype(np.float32))


_LOG = re.compile(r'Average PSNR: \S+ dB  SSIM: \S+  MAE: \S+ over (\d+) slices \(global range \[\S+, \S+\]\)  LPIPS: (\S+)')


def test_driver_device_metrics_with_lpips(tmp_path):
    """`python -m mudiff_hip.driver --device_metrics --lpips_weights` on the s32 config: the logged LPIPS is the restatement's on the
    exported PNGs, at the printed precision."""
    from PIL import Image
    data = tmp_path / 'data'
    _write_volumes(str(data), n=7, hw=32, seed=5)
    cfg = O.default_config(**SMALL_CFGS['s32'])
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG, os.environ.get('PYTHONPATH', '')]), MUD_DETERMINISTIC='1')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    out = tmp_path / 'out'
    os.makedirs(out / 'exp7')
    for which, name in (('g1', 'gen_diffusive_1'), ('g2', 'gen_diffusive_2')):
        torch.save({'module.' + k: v for k, v in O.make_state_dict(cfg, which, 1234).items()}, out / 'exp7' / f'{name}.pth')
    sd = seeded_weights(21)
    torch.save(sd, tmp_path / 'lpips_alex.pth')
    cmd = [sys.executable, '-m', 'mudiff_hip.driver', '--input_path', str(data), '--output_path', str(out), '--exp', 'exp7',
           '--target_modality', 'T2', '--image_size', '32', '--num_channels_dae', '32', '--ch_mult', '1', '2', '4',
           '--attn_resolutions', '16', '--batch_size', '4', '--device_metrics', '--lpips_weights', str(tmp_path / 'lpips_alex.pth')]
    p = subprocess.run(cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    m = _LOG.search(p.stderr)
    assert m, p.stderr[-2000:]
    assert m.group(1) == '7'
    png = out / 'generated_samples'
    names = sorted(os.listdir(png / 'pred'))
    assert len(names) == 7
    p8 = np.stack([np.array(Image.open(png / 'pred' / f).convert('L')) for f in names])
    g8 = np.stack([np.array(Image.open(png / 'gt' / f.replace('pred', 'gt')).convert('L')) for f in names])
    ref = lpips_taps(p8, g8, sd).sum(1).mean()
    assert abs(float(m.group(2)) - ref) <= 0.5e-6 + 1e-5 * ref + 1e-12, (m.group(2), ref)


# ---------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _worker(rank, world, port, sd, preds, gts, q):
    for p in (REPO, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from mudiff_hip import metrics
    from mudiff_hip.lpips_net import LpipsAlex
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        net = LpipsAlex.from_state_dict(sd)                     # every rank loads its own copy
        lo, hi = (0, 3) if rank == 0 else (3, preds.shape[0])
        res = metrics.score_distributed(lo, preds[lo:hi].to(DEV), gts[lo:hi].to(DEV), group=None, lpips=net)
        q.put((rank, None if res is None else (res['lpips'], res['lpips_per_slice'], res['psnr_per_slice'])))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_lpips_matches_one_rank():
    from mudiff_hip import metrics
    from mudiff_hip.lpips_net import LpipsAlex
    sd = seeded_weights(31)
    rng = np.random.default_rng(9)
    gts = torch.from_numpy(rng.uniform(-1, 1, (5, 40, 48)).astype(np.float32))
    preds = torch.clamp(gts + 0.1 * torch.from_numpy(rng.standard_normal((5, 40, 48)).astype(np.float32)), -1.2, 1.1)
    single = metrics.score_device(preds.to(DEV), gts.to(DEV), lpips=LpipsAlex.from_state_dict(sd))
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, sd, preds, gts, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in range(2)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[1][1] is None
    lp, per, psnr = res[0][1]
    assert np.array_equal(per, single['lpips_per_slice']) and lp == single['lpips']
    assert np.array_equal(psnr, single['psnr_per_slice'])
