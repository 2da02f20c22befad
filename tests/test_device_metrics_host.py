"""CPU: the host side of the on-device metrics (mudiff_hip.metrics) - the integer-window restatement of the SSIM the kernel
evaluates, the merge of per-rank sums, the 2-rank gloo range reduction and gather, and the CLI's argument errors."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import PKG, REPO


# ---------------------------------------------------------------------------------------------------
def _box7(x):
    """7x7 box sums of an int64 image over the (H-6) x (W-6) window positions (exact)."""
    H, W = x.shape
    c = np.zeros((H + 1, W + 1), np.int64)
    c[1:, 1:] = x.cumsum(0).cumsum(1)
    return c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]


def host_sums(p8, g8):
    """fp64 restatement of one slice of mud_slice_metrics_u8 from exact integer window sums -> (sse, sae, ssim_sum)."""
    q, r = p8.astype(np.int64), g8.astype(np.int64)
    Sq, Sr, Sqq, Srr, Sqr = _box7(q), _box7(r), _box7(q * q), _box7(r * r), _box7(q * r)
    a1, b1 = 2 * Sq * Sr, Sq * Sq + Sr * Sr
    a2, b2 = 2 * (49 * Sqr - Sq * Sr), (49 * Sqq - Sq * Sq) + (49 * Srr - Sr * Sr)
    C1 = (0.01 * 0.01) * (12495.0 * 12495.0)
    C2 = (0.03 * 0.03) * (49.0 * 48.0 * 255.0 * 255.0)
    s = ((a1 + C1) * (a2 + C2)) / ((b1 + C1) * (b2 + C2))
    d = r - q
    return int((d * d).sum()), int(np.abs(d).sum()), float(s.sum())


def host_metrics(p8, g8):
    """driver.export_and_score's per-slice scores of one uint8 pair -> (psnr, ssim, mae)."""
    from mudiff_hip import driver
    pn, gn = p8.astype(np.float32) / 255.0, g8.astype(np.float32) / 255.0
    return driver.psnr(gn, pn), driver.ssim(gn, pn), float(np.mean(np.abs(gn - pn)))


def test_integer_window_restatement_matches_the_host_ssim():
    """The exactness argument of csrc/metrics.hip on the host: the SSIM from integer window sums agrees with driver.ssim (fp32 k/255
    through scipy filters) to well inside the device tolerance, and PSNR / MAE from the integer sums with the host's."""
    from mudiff_hip import metrics
    rng = np.random.default_rng(3)
    for H, W in ((7, 7), (37, 53), (64, 64)):
        g8 = rng.integers(0, 256, (H, W), dtype=np.uint8)
        p8 = np.clip(g8.astype(np.int64) + rng.integers(-20, 21, (H, W)), 0, 255).astype(np.uint8)
        sse, sae, ss = host_sums(p8, g8)
        (ps,), (sm,), (ma,) = metrics.per_slice_values([sse], [sae], [ss], H, W)
        hp, hs, hm = host_metrics(p8, g8)
        assert abs(ps - hp) <= 1e-5 and abs(sm - hs) <= 1e-8 and abs(ma - hm) <= 1e-7, (H, W, ps - hp, sm - hs, ma - hm)
    same = rng.integers(0, 256, (9, 9), dtype=np.uint8)
    sse, sae, ss = host_sums(same, same)
    assert (sse, sae) == (0, 0) and ss == pytest.approx(9.0, abs=1e-12)
    assert metrics.per_slice_values([0], [0], [ss], 9, 9)[0] == [float('inf')]


def _parts(n=10, H=32, W=40, seed=0):
    rng = np.random.default_rng(seed)
    sse = rng.integers(0, 255 * 255 * H * W // 50, n).astype(np.int64)
    sse[4] = 0                                                        # identical images: PSNR inf
    sae = rng.integers(0, 255 * H * W // 20, n).astype(np.int64)
    ss = rng.uniform(0.2, 1.0, n) * (H - 6) * (W - 6)
    return sse, sae, ss


def test_combine_shards_matches_the_single_shard_in_any_order():
    from mudiff_hip import metrics
    sse, sae, ss = _parts()
    part = lambda lo, hi: dict(lo=lo, sse=sse[lo:hi], sae=sae[lo:hi], ssim_sum=ss[lo:hi], H=32, W=40)     # noqa: E731
    one = metrics.combine_shards([part(0, 10)])
    assert one['count'] == 10 and one['psnr'] == float('inf')
    ps, sm, ma = metrics.per_slice_values(sse, sae, ss, 32, 40)
    assert one['ssim'] == sum(sm) / 10 and one['mae'] == sum(ma) / 10
    assert list(one['psnr_per_slice']) == ps
    for parts in ([part(3, 7), part(7, 7), part(0, 3), part(7, 10)], [part(7, 10), part(0, 7)], [part(0, 0), part(0, 10), part(10, 10)]):
        got = metrics.combine_shards(parts)
        assert {k: got[k] for k in ('psnr', 'ssim', 'mae', 'count')} == {k: one[k] for k in ('psnr', 'ssim', 'mae', 'count')}
        for k in ('psnr_per_slice', 'ssim_per_slice', 'mae_per_slice', 'sse', 'sae', 'ssim_sum'):
            assert np.array_equal(got[k], one[k]), k
    finite = metrics.combine_shards([dict(lo=0, sse=sse[5:], sae=sae[5:], ssim_sum=ss[5:], H=32, W=40)])
    assert np.isfinite(finite['psnr']) and finite['count'] == 5
    with pytest.raises(ValueError, match='tile'):
        metrics.combine_shards([part(0, 3), part(4, 10)])
    assert metrics.combine_shards([part(5, 5)])['count'] == 0


# ---------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    for p in (REPO, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from mudiff_hip import metrics
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        ranges = {0: [-0.5, 0.75], 1: [-0.875, 0.25], 2: [float('inf'), -float('inf')]}   # rank 2: an empty shard
        got = metrics.reduce_range(torch.tensor(ranges[rank], dtype=torch.float32))
        const = metrics.reduce_range(torch.tensor([0.5, 0.5] if rank < 2 else [float('inf'), -float('inf')]))
        try:
            metrics.reduce_range(torch.tensor([float('nan'), float('nan')] if rank == 1 else [0.0, 1.0]))
            nan = 'no error'
        except ValueError:
            nan = 'ValueError'
        sse, sae, ss = _parts()
        shards = {0: (0, 6), 1: (6, 10), 2: (10, 10)}
        lo, hi = shards[rank]
        parts = metrics.gather_parts(dict(lo=lo, sse=sse[lo:hi], sae=sae[lo:hi], ssim_sum=ss[lo:hi], H=32, W=40))
        res = None if parts is None else {k: metrics.combine_shards(parts)[k] for k in ('psnr', 'ssim', 'mae', 'count')}
        q.put((rank, got, const, nan, res))
    finally:
        dist.destroy_process_group()


def test_three_rank_gloo_range_reduce_and_gather():
    from mudiff_hip import metrics
    world = 3
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in range(world)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(r[1] == (-0.875, 0.75) for r in res)                  # MIN / MAX over ranks, the empty shard neutral
    assert all(r[2] == (0.0, 1.0) for r in res)                       # constant images: the host path's (0, 1) fallback
    assert all(r[3] == 'ValueError' for r in res)                     # a NaN on one rank stops every rank
    sse, sae, ss = _parts()
    single = {k: metrics.combine_shards([dict(lo=0, sse=sse, sae=sae, ssim_sum=ss, H=32, W=40)])[k] for k in ('psnr', 'ssim', 'mae', 'count')}
    assert res[0][4] == single and res[1][4] is None and res[2][4] is None


# ---------------------------------------------------------------------------------------------------
def test_metrics_cli_argument_errors(tmp_path):
    from mudiff_hip import metrics
    (tmp_path / 'gt').mkdir()
    (tmp_path / 'pred').mkdir()
    (tmp_path / 'gt' / 'a.png').write_bytes(b'')
    (tmp_path / 'pred' / 'b.png').write_bytes(b'')
    os.makedirs(tmp_path / 'pred' / 'a.png')                          # a directory of that name is not a file
    with pytest.raises(RuntimeError, match='No matching image files'):
        metrics.main(['--gt_dir', str(tmp_path / 'gt'), '--pred_dir', str(tmp_path / 'pred')])
    with pytest.raises(SystemExit):
        metrics.main(['--gt_dir', str(tmp_path / 'gt')])
    assert metrics.common_files(str(tmp_path / 'gt'), str(tmp_path / 'gt')) == ['a.png']


def test_driver_flag_defaults_off():
    from mudiff_hip import driver
    assert driver.build_parser().parse_args([]).device_metrics is False
    assert driver.build_parser().parse_args(['--device_metrics']).device_metrics is True
