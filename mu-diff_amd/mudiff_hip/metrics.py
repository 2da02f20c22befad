"""On-device PSNR / SSIM / MAE of 8-bit quantised slices (the driver's --device_metrics, and a device restatement of the
reference's tools/metric_calc.py).

The host path (driver.export_and_score) quantises every slice with numpy, runs five scipy filters per slice for the SSIM and
gathers every fp32 slice on rank 0.  Here the GPU does the work (csrc/metrics.hip, through mudiff_hip.ops):

- ops.value_range: the global min / max of a rank's predictions and targets (ranks combine with one MAX all_reduce);
- ops.quantize_u8: the 8-bit images, bit-identical to driver.to_uint8;
- ops.slice_metrics_u8: per slice the exact integer sums sse = sum (g-p)^2 and sae = sum |g-p|, and the fp64 sum of the per-pixel
  SSIM (skimage defaults, as driver.ssim) over the interior, from exact integer window sums.

Final values come from those sums on the host, averaged in slice order as export_and_score averages them:
psnr = 10 log10(255^2 H W / sse) (inf for identical images), ssim = ssim_sum / ((H-6)(W-6)), mae = sae / (255 H W).

LPIPS-alex (the fourth number of metric_calc) is optional: pass `lpips=` a mudiff_hip.lpips_net.LpipsAlex built from the user's
weight files (ops.lpips_u8 on the same 8-bit images; per-slice fp64 values, averaged in slice order like the others).

    python -m mudiff_hip.metrics --gt_dir results/generated_samples/gt --pred_dir results/generated_samples/pred
    python -m mudiff_hip.metrics --gt_dir ... --pred_dir ... --lpips_weights alex_lpips.pth            # + 'Average LPIPS'
    python -m mudiff_hip.metrics --gt_dir ... --pred_dir ... --lpips_weights alexnet.pth --lpips_lin alex.pth

Without --lpips_weights the CLI prints PSNR, SSIM and MAE only."""
from __future__ import annotations

import argparse
import math
import os

import numpy as np
import torch


# ---------------------------------------------------------------------------------------------------
def per_slice_values(sse, sae, ssim_sum, H, W):
    """Per-slice (psnr, ssim, mae) python-float lists from the integer / fp64 sums of slices of H x W pixels."""
    sse, sae, ssim_sum = np.asarray(sse, np.int64), np.asarray(sae, np.int64), np.asarray(ssim_sum, np.float64)
    peak = 255.0 * 255.0 * H * W
    psnr = [float('inf') if e == 0 else 10.0 * math.log10(peak / float(e)) for e in sse.tolist()]
    ssim = (ssim_sum / float((H - 6) * (W - 6))).tolist()
    mae = (sae.astype(np.float64) / (255.0 * H * W)).tolist()
    return psnr, ssim, mae


def average(psnr, ssim, mae):
    """Means in slice order, accumulated one slice at a time like driver.export_and_score."""
    ps = ss = ma = 0.0
    for p, s, m in zip(psnr, ssim, mae):
        ps += p
        ss += s
        ma += m
    n = max(len(psnr), 1)
    return dict(psnr=ps / n, ssim=ss / n, mae=ma / n, count=len(psnr))


def combine_shards(parts):
    """Rank 0's merge of the ranks' per-slice sums.  `parts`: dicts (lo, sse, sae, ssim_sum, H, W [, lpips]), one per rank, in any
    order; empty shards allowed.  The shards must tile [0, total) without gaps.  -> dict(psnr, ssim, mae, count) plus the per-slice
    lists, in global slice order; with `lpips` (per-slice fp64, on every non-empty part or on none) also lpips (the mean in slice
    order) and lpips_per_slice."""
    parts = sorted((p for p in parts if len(p['sse'])), key=lambda p: p['lo'])
    with_lpips = [p.get('lpips') is not None for p in parts]
    if any(with_lpips) and not all(with_lpips):
        raise ValueError('some shards carry LPIPS values and others do not')
    psnr, ssim, mae, sse, sae, ssim_sum = [], [], [], [], [], []
    nxt = 0
    for p in parts:
        if p['lo'] != nxt:
            raise ValueError(f'shards do not tile the slice range: expected a shard at {nxt}, got one at {p["lo"]}')
        a, b, c = per_slice_values(p['sse'], p['sae'], p['ssim_sum'], p['H'], p['W'])
        psnr += a
        ssim += b
        mae += c
        sse += np.asarray(p['sse'], np.int64).tolist()
        sae += np.asarray(p['sae'], np.int64).tolist()
        ssim_sum += np.asarray(p['ssim_sum'], np.float64).tolist()
        nxt += len(p['sse'])
    res = average(psnr, ssim, mae)
    res.update(psnr_per_slice=np.array(psnr), ssim_per_slice=np.array(ssim), mae_per_slice=np.array(mae),
               sse=np.array(sse, np.int64), sae=np.array(sae, np.int64), ssim_sum=np.array(ssim_sum, np.float64))
    if parts and all(with_lpips):
        per = []
        for p in parts:
            v = np.asarray(p['lpips'], np.float64).reshape(-1)
            if len(v) != len(p['sse']):
                raise ValueError(f'shard at {p["lo"]}: {len(v)} LPIPS values for {len(p["sse"])} slices')
            per += v.tolist()
        acc = 0.0
        for v in per:                                  # one slice at a time, like average()
            acc += v
        res.update(lpips=acc / len(per), lpips_per_slice=np.array(per, np.float64))
    return res


# ---------------------------------------------------------------------------------------------------
def reduce_range(mm, group=None):
    """[min, max] of this rank (tensor of 2, any device) -> the global (gmin, gmax) as python floats, with the host path's (0, 1)
    fallback for an empty or constant range.  Over ranks: ONE all_reduce of [-min, max, nan] with MAX, so that a NaN on any rank
    makes every rank raise ValueError (instead of one rank raising while the others wait in a collective)."""
    import torch.distributed as dist
    lo, hi = (float(v) for v in mm.detach().double().cpu().tolist())
    nan = math.isnan(lo) or math.isnan(hi)
    t = torch.tensor([0.0, 0.0, 1.0] if nan else [-lo, hi, 0.0], dtype=torch.float64, device=mm.device)
    if dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    nlo, hi, nan = t.tolist()
    if nan:
        raise ValueError('the predictions or targets contain NaN: no intensity range for the 8-bit export')
    gmin, gmax = -nlo, hi
    if gmax <= gmin:                                  # constant (or empty) images: engine/test.py:377-378
        gmin, gmax = 0.0, 1.0
    return gmin, gmax


def gather_parts(part, group=None):
    """Every rank's `part` (a small picklable object) on rank 0 -> list (rank 0) or None; [part] without a process group."""
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return [part]
    parts = [None] * dist.get_world_size(group)
    dst = 0
    dist.gather_object(part, parts if dist.get_rank() == dst else None, dst=dst, group=group)
    return parts if dist.get_rank() == dst else None


def write_pngs(pred8, gt8, save_dir, lo=0):
    """<save_dir>/pred/pred_{lo+i:05d}.png and gt/gt_{lo+i:05d}.png from uint8 [n, H, W] arrays (global slice numbers)."""
    from PIL import Image
    os.makedirs(os.path.join(save_dir, 'pred'), exist_ok=True)
    os.makedirs(os.path.join(save_dir, 'gt'), exist_ok=True)
    for i, (p, g) in enumerate(zip(pred8, gt8)):
        Image.fromarray(p).save(os.path.join(save_dir, 'pred', f'pred_{lo + i:05d}.png'))
        Image.fromarray(g).save(os.path.join(save_dir, 'gt', f'gt_{lo + i:05d}.png'))


def _as_slices(t):
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3:
        raise ValueError(f'expected slices [n, H, W], got {tuple(t.shape)}')
    return t.float().contiguous()


def score_shard(lo, preds, gts, save_dir=None, group=None, return_images=False, lpips=None):
    """One rank's part of a (possibly multi-rank) device evaluation: its slices [lo, lo+n) as device fp32 [n, H, W] tensors.
    Global range over all ranks, 8-bit quantisation and PNG export (global slice numbers) of this shard, per-slice sums.
    -> (gmin, gmax, part) with part = dict(lo, sse, sae, ssim_sum, H, W) (host numpy) [+ pred_u8 / gt_u8 device tensors]; with
    `lpips` (an LpipsAlex) the part also carries lpips, the per-slice LPIPS-alex of the 8-bit images (fp64)."""
    from . import ops
    preds, gts = _as_slices(preds), _as_slices(gts)
    if preds.shape != gts.shape:
        raise ValueError(f'predictions {tuple(preds.shape)} and targets {tuple(gts.shape)} differ in shape')
    gmin, gmax = reduce_range(ops.value_range(preds, gts), group)
    n, H, W = preds.shape
    part = dict(lo=int(lo), sse=np.zeros(0, np.int64), sae=np.zeros(0, np.int64), ssim_sum=np.zeros(0, np.float64), H=int(H), W=int(W))
    if lpips is not None:
        part.update(lpips=np.zeros(0, np.float64))
    if n == 0:
        return gmin, gmax, part
    p8, g8 = ops.quantize_u8(preds, gmin, gmax), ops.quantize_u8(gts, gmin, gmax)
    sse, sae, ssim_sum = ops.slice_metrics_u8(p8, g8)
    if lpips is not None:
        from .lpips_net import lpips_totals
        part.update(lpips=lpips_totals(ops.lpips_u8(p8, g8, lpips.to(preds.device)).cpu().numpy()))
    if save_dir is not None:
        write_pngs(p8.cpu().numpy(), g8.cpu().numpy(), save_dir, lo)
    part.update(sse=sse.cpu().numpy(), sae=sae.cpu().numpy(), ssim_sum=ssim_sum.cpu().numpy())
    if return_images:
        part.update(pred_u8=p8, gt_u8=g8)
    return gmin, gmax, part


def score_device(preds, gts, save_dir=None, return_images=False, lpips=None):
    """driver.export_and_score on the GPU: device fp32 predictions and targets [n, H, W] (n >= 1) -> dict(psnr, ssim, mae, count,
    global_min, global_max) with the same values (the 8-bit images bit-identical), plus the per-slice values (psnr_per_slice,
    ssim_per_slice, mae_per_slice) and sums (sse, sae, ssim_sum); with `return_images` also the uint8 images (pred_u8, gt_u8,
    device tensors); with `lpips` (an LpipsAlex) also lpips and lpips_per_slice.  Raises ValueError on NaN input."""
    if preds.shape[0] == 0:
        raise ValueError('score_device: no slices to score')
    gmin, gmax, part = score_shard(0, preds, gts, save_dir=save_dir, return_images=return_images, lpips=lpips)
    res = combine_shards([part])
    res.update(global_min=gmin, global_max=gmax)
    if return_images:
        res.update(pred_u8=part['pred_u8'], gt_u8=part['gt_u8'])
    return res


def score_distributed(lo, preds, gts, save_dir=None, group=None, lpips=None):
    """The driver's --device_metrics over all ranks: every rank quantises, exports and scores its own shard (LPIPS too, with its
    own copy of the weights, when `lpips` is given); rank 0 gathers only (lo, per-slice values) and combines them in global slice
    order.  -> result dict on rank 0, None elsewhere."""
    gmin, gmax, part = score_shard(lo, preds, gts, save_dir=save_dir, group=group, lpips=lpips)
    parts = gather_parts(part, group)
    if parts is None:
        return None
    res = combine_shards(parts)
    if res['count'] == 0:
        raise ValueError('no slices to score')
    res.update(global_min=gmin, global_max=gmax)
    return res


# ---------------------------------------------------------------------------------------------------
def common_files(gt_dir, pred_dir):
    """tools/metric_calc.py:20-25: regular files present in both directories, sorted by name; none is a RuntimeError."""
    gt = sorted(f for f in os.listdir(gt_dir) if os.path.isfile(os.path.join(gt_dir, f)))
    pred = set(f for f in os.listdir(pred_dir) if os.path.isfile(os.path.join(pred_dir, f)))
    common = [f for f in gt if f in pred]
    if not common:
        raise RuntimeError('No matching image files found in the provided directories.')
    return common


def score_dirs(gt_dir, pred_dir, batch_size=64, device='cuda', lpips=None):
    """PSNR / SSIM / MAE of the grayscale ('L') images with the same name in both directories, scored on the device in batches of
    `batch_size` (runs of equal shape).  -> dict(psnr, ssim, mae, count) + per-slice values, in file-name order; with `lpips` (an
    LpipsAlex) also lpips and lpips_per_slice."""
    from PIL import Image
    from . import ops
    files = common_files(gt_dir, pred_dir)
    if batch_size < 1:
        raise ValueError('batch_size must be >= 1')
    device = torch.device(device)
    if lpips is not None:
        from .lpips_net import lpips_totals
        lpips = lpips.to(device)
    parts, lo = [], 0
    for b0 in range(0, len(files), batch_size):
        names = files[b0:b0 + batch_size]
        gt = [np.array(Image.open(os.path.join(gt_dir, f)).convert('L'), dtype=np.uint8) for f in names]
        pr = [np.array(Image.open(os.path.join(pred_dir, f)).convert('L'), dtype=np.uint8) for f in names]
        i = 0
        while i < len(names):                          # a run of equally sized images is one launch
            j = i + 1
            while j < len(names) and gt[j].shape == gt[i].shape:
                j += 1
            for k in range(i, j):
                if pr[k].shape != gt[k].shape:
                    raise ValueError(f'{names[k]}: prediction {pr[k].shape} and ground truth {gt[k].shape} differ in size')
            H, W = gt[i].shape
            g8 = torch.from_numpy(np.stack(gt[i:j])).to(device)
            p8 = torch.from_numpy(np.stack(pr[i:j])).to(device)
            sse, sae, ssim_sum = ops.slice_metrics_u8(p8, g8)
            parts.append(dict(lo=lo, sse=sse.cpu().numpy(), sae=sae.cpu().numpy(), ssim_sum=ssim_sum.cpu().numpy(), H=H, W=W))
            if lpips is not None:
                parts[-1].update(lpips=lpips_totals(ops.lpips_u8(p8, g8, lpips).cpu().numpy()))
            lo += j - i
            i = j
    return combine_shards(parts)


def build_parser():
    p = argparse.ArgumentParser(description='Compute PSNR, SSIM and MAE (and LPIPS-alex with --lpips_weights) between prediction and '
                                            'ground truth images on the GPU (tools/metric_calc.py).')
    p.add_argument('--gt_dir', type=str, required=True, help='Path to directory of ground truth images (png format).')
    p.add_argument('--pred_dir', type=str, required=True, help='Path to directory of predicted images.')
    p.add_argument('--batch_size', type=int, default=64, help='images per device launch')
    add_lpips_flags(p)
    return p


def add_lpips_flags(p):
    p.add_argument('--lpips_weights', type=str, default=None,
                   help='LPIPS-alex weights: a saved lpips.LPIPS(net=\'alex\').state_dict(), or a torchvision AlexNet state dict '
                        'together with --lpips_lin (mudiff_hip.lpips_net)')
    p.add_argument('--lpips_lin', type=str, default=None, help="lpips's weights/v0.1/alex.pth (the lin layers), with an AlexNet --lpips_weights")


def check_lpips_flags(p, args):
    if args.lpips_lin is not None and args.lpips_weights is None:
        p.error('--lpips_lin needs --lpips_weights')


def load_lpips(args):
    """The LpipsAlex of --lpips_weights / --lpips_lin, or None."""
    if args.lpips_weights is None:
        return None
    from .lpips_net import LpipsAlex
    return LpipsAlex.from_files(args.lpips_weights, args.lpips_lin)


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    check_lpips_flags(p, args)
    return args


def main(argv=None):
    args = parse_args(argv)
    res = score_dirs(args.gt_dir, args.pred_dir, args.batch_size, lpips=load_lpips(args))
    print(f"Average PSNR: {res['psnr']:.4f} dB")
    print(f"Average SSIM: {res['ssim']:.4f}")
    print(f"Average MAE: {res['mae']:.6f}")
    if 'lpips' in res:
        print(f"Average LPIPS: {res['lpips']:.6f}")
    return res


if __name__ == '__main__':
    main()
