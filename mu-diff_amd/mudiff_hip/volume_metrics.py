"""On-device scoring of a predicted volume against its ground truth: masked 3D SSIM, PSNR and MAE per region, per-plane curves, the
2D driver's 8-bit slice metrics, and (with an ensemble's std volume) whether the std points at the errors.  DESIGN.md section 5.9.

Definitions (every score is taken on the slab: the planes s0..s1 that volume.extract_center_slices(z, slice_half_range) selects):
- prediction: the fp32 values in [0, 1] as written to predicted_<t>.nii.gz;
- ground truth: robust_minmax_to_minus1_1 of the raw GT volume (whole-volume percentiles, like the inputs), then ops.to_range_0_1;
  with norm='zscore' (--norm zscore) volume.zscore_to_minus1_1 instead, like the inputs of that mode; the report then has "norm": "zscore";
- regions (bit k of a uint8 per voxel): slab = every voxel, brain = raw GT != 0, and with a label volume tumor = label != 0 and
  healthy = brain and not tumor;
- SSIM3D: skimage's structural_similarity carried to three axes (uniform 7x7x7 window, sample covariance 343/342, K1 = 0.01,
  K2 = 0.03, data_range 1), evaluated at the voxels whose whole window lies in the slab; a region's SSIM3D is the mean of that map over
  its interior voxels.  For `slab` it equals structural_similarity(gt_slab, pred_slab, data_range=1.0) on the 3D arrays;
- PSNR = 10 log10(1 / mse) (inf when mse is 0) and MAE = mean |p - g| over all of the region's voxels;
- per-plane curves: the same per slab plane (a plane's SSIM3D: the mean of the 3D map over that plane's interior voxels);
- slice2d: metrics.score_device on the slab's planes (the reference's 8-bit global-range protocol, comparable with the 2D driver);
- uncertainty (with a std volume): per region the mean std and the Pearson correlation of std and |mean - gt|.
An empty region (no voxels, or no interior voxels for SSIM3D) reports None (null in the JSON).

The sums come from csrc/volume_metrics.hip (ops.volume_metrics) per plane and region; the totals add them on the host in fp64 in
plane order, so every number is a fixed function of the inputs.

    python -m mudiff_hip.volume_metrics --pred predicted_t1ce.nii.gz --gt t1ce.nii.gz [--mask seg.nii.gz] [--std predicted_t1ce_std.nii.gz]
                                        [--slice_half_range 80] [--json metrics.json]
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import warnings

import numpy as np
import torch

REGIONS = ('slab', 'brain', 'tumor', 'healthy')        # bit k of the region mask is REGIONS[k]
MIN_EXTENT = 7                                         # the SSIM window
# a variance below this fraction of the mean square is rounding noise of the raw moments: the correlation is reported as null
VAR_FLOOR = 1e-10


# ---------------------------------------------------------------------------------------------------
# host-side preparation
# ---------------------------------------------------------------------------------------------------
def slab_range(z, slice_half_range):
    """The planes s0..s1 that volume.extract_center_slices picks from a volume of z planes."""
    c = int(z) // 2
    return max(0, c - int(slice_half_range)), min(int(z) - 1, c + int(slice_half_range))


def check_shapes(pred_shape, gt_shape, mask_shape=None, slice_half_range=80, std_shape=None):
    """ValueError unless prediction, GT, mask and std share one 3D shape whose slab is at least 7 x 7 x 7.  -> (s0, s1)."""
    pred_shape, gt_shape = tuple(pred_shape), tuple(gt_shape)
    if len(gt_shape) != 3:
        raise ValueError(f'the ground truth must be a 3D volume, got shape {gt_shape}')
    if pred_shape != gt_shape:
        raise ValueError(f'prediction {pred_shape} and ground truth {gt_shape} differ in shape')
    if mask_shape is not None and tuple(mask_shape) != gt_shape:
        raise ValueError(f'the label mask {tuple(mask_shape)} and the ground truth {gt_shape} differ in shape')
    if std_shape is not None and tuple(std_shape) != gt_shape:
        raise ValueError(f'the std volume {tuple(std_shape)} and the ground truth {gt_shape} differ in shape')
    if min(gt_shape[:2]) < MIN_EXTENT:
        raise ValueError(f'in-plane size {gt_shape[:2]} is below {MIN_EXTENT} (the SSIM window)')
    s0, s1 = slab_range(gt_shape[2], slice_half_range)
    if s1 - s0 + 1 < MIN_EXTENT:
        raise ValueError(f'the slab (planes {s0}..{s1}, slice_half_range {slice_half_range}) has {s1 - s0 + 1} planes: at least '
                         f'{MIN_EXTENT} are needed for the 7x7x7 SSIM window')
    return s0, s1


def slab_planes(vol, s0, s1, dtype=np.float32):
    """[X, Y, Z] volume -> its slab as a contiguous [s1 - s0 + 1, X, Y] array (planes contiguous, like the pipeline's slices)."""
    return np.ascontiguousarray(np.moveaxis(np.asarray(vol)[:, :, s0:s1 + 1], 2, 0), dtype=dtype)


def region_mask(gt_raw, label=None):
    """uint8 region bits of the voxels of a raw GT array (any shape) and an optional label array of the same shape:
    bit 0 slab (every voxel), bit 1 brain (gt != 0), and with `label` bit 2 tumor (label != 0), bit 3 healthy (brain, not tumor).
    -> (mask, region names)."""
    brain = np.asarray(gt_raw) != 0
    m = np.ones(brain.shape, np.uint8) | (brain.astype(np.uint8) << 1)
    if label is None:
        return m, REGIONS[:2]
    tumor = np.asarray(label) != 0
    m |= (tumor.astype(np.uint8) << 2) | ((brain & ~tumor).astype(np.uint8) << 3)
    return m, REGIONS


# ---------------------------------------------------------------------------------------------------
# sums -> report
# ---------------------------------------------------------------------------------------------------
def _psnr(n, sse):
    if n == 0:
        return None
    return float('inf') if sse == 0 else 10.0 * math.log10(n / sse)


def _values(q):
    """Scores of one region from its fp64 sums (one row of MUD_VM_NQ)."""
    from .ops import VM_N, VM_N_INT, VM_SAE, VM_SSE, VM_SSIM
    n, ni = int(q[VM_N]), int(q[VM_N_INT])
    return dict(voxels=n, interior_voxels=ni, psnr=_psnr(n, float(q[VM_SSE])), ssim3d=float(q[VM_SSIM]) / ni if ni else None,
                mae=float(q[VM_SAE]) / n if n else None, mse=float(q[VM_SSE]) / n if n else None, sse=float(q[VM_SSE]),
                sae=float(q[VM_SAE]))


def _uncertainty(q):
    """Mean std and Pearson r(std, |err|) of one region from its raw moments; r is None when either variance is (numerically) 0."""
    from .ops import VM_N, VM_SAE, VM_SS, VM_SS2, VM_SSE, VM_SSE_STD
    n = float(q[VM_N])
    if n == 0:
        return dict(mean_std=None, pearson_r=None)
    ms, me = float(q[VM_SS]) / n, float(q[VM_SAE]) / n
    s2, e2 = float(q[VM_SS2]) / n, float(q[VM_SSE]) / n
    vs, ve = s2 - ms * ms, e2 - me * me
    r = None
    if vs > VAR_FLOOR * s2 and ve > VAR_FLOOR * e2:
        r = (float(q[VM_SSE_STD]) / n - ms * me) / math.sqrt(vs * ve)
    return dict(mean_std=ms, pearson_r=r)


def summarize(sums, names, first_plane=0, has_std=False):
    """Report of per-plane sums (array-like [planes, len(names), MUD_VM_NQ], fp64; ops.volume_metrics) -> dict with
    regions (names), metrics {name: voxels, interior_voxels, psnr, ssim3d, mae, mse, sse, sae}, per_plane {plane: [...], name: {psnr,
    ssim3d, mae}} and, with `has_std`, uncertainty {name: mean_std, pearson_r}.  Region totals add the planes in plane order (fp64)."""
    sums = np.asarray(sums, np.float64)
    if sums.ndim != 3 or sums.shape[1] != len(names):
        raise ValueError(f'sums of shape {sums.shape} do not hold {len(names)} regions')
    P = sums.shape[0]
    rep = dict(regions=list(names), metrics={}, per_plane=dict(plane=list(range(int(first_plane), int(first_plane) + P))))
    unc = {}
    for k, name in enumerate(names):
        tot = np.zeros(sums.shape[2], np.float64)
        for z in range(P):
            tot = tot + sums[z, k]
        rep['metrics'][name] = _values(tot)
        per = [_values(sums[z, k]) for z in range(P)]
        rep['per_plane'][name] = {key: [v[key] for v in per] for key in ('psnr', 'ssim3d', 'mae')}
        if has_std:
            unc[name] = _uncertainty(tot)
    if has_std:
        rep['uncertainty'] = unc
    return rep


def _fmt(v, spec):
    if v is None:
        return 'n/a'
    return 'inf' if math.isinf(v) else format(v, spec)


def format_lines(rep):
    """The printed summary: one line per region, the slice2d line and the uncertainty lines."""
    lines = []
    for name in rep['regions']:
        m = rep['metrics'][name]
        lines.append(f"[metrics] {name}: PSNR {_fmt(m['psnr'], '.4f')} dB | SSIM3D {_fmt(m['ssim3d'], '.6f')} | MAE {_fmt(m['mae'], '.6f')} | "
                     f"voxels {m['voxels']}")
    s = rep.get('slice2d')
    if s is not None:
        lines.append(f"[metrics] slice2d (8-bit, {s['count']} planes): PSNR {_fmt(s['psnr'], '.4f')} dB | SSIM {_fmt(s['ssim'], '.4f')} | "
                     f"MAE {_fmt(s['mae'], '.6f')}")
    for name, u in rep.get('uncertainty', {}).items():
        lines.append(f"[metrics] uncertainty {name}: mean std {_fmt(u['mean_std'], '.6f')} | r(std, |err|) {_fmt(u['pearson_r'], '.4f')}")
    return lines


def write_json(rep, path):
    """The report as JSON (PSNR inf is written as Infinity, an empty region's scores as null)."""
    with open(path, 'w') as f:
        json.dump(rep, f, indent=1)
    return path


# ---------------------------------------------------------------------------------------------------
# device scoring
# ---------------------------------------------------------------------------------------------------
def _check_finite(a, b=None, what='the prediction or the ground truth'):
    from . import ops
    lo, hi = ops.value_range(a, b).cpu().tolist()
    if math.isnan(lo) or math.isnan(hi):
        raise ValueError(f'{what} contains NaN: it cannot be scored')


def score_volume(pred, gt, region, std=None, names=REGIONS, first_plane=0):
    """Scores of a slab: device tensors [Z', X, Y] (planes contiguous) - pred and gt fp32 in [0, 1], region the uint8 bits of `names`
    (region_mask), std the ensemble's fp32 std or None.  -> summarize(...)'s report plus slice2d (metrics.score_device on the planes:
    psnr, ssim, mae, count, global_min, global_max).  ValueError, before the scoring kernels run, on a shape below 7 x 7 x 7, on
    mismatched shapes and on NaN input."""
    from . import metrics, ops
    names = tuple(names)
    ts = [('pred', pred), ('gt', gt), ('region', region)] + ([] if std is None else [('std', std)])
    if pred.dim() != 3 or any(tuple(t.shape) != tuple(pred.shape) for _, t in ts):
        raise ValueError('score_volume: need [Z, X, Y] tensors of one shape, got ' + ', '.join(f'{k} {tuple(t.shape)}' for k, t in ts))
    if min(pred.shape) < MIN_EXTENT:
        raise ValueError(f'score_volume: the slab {tuple(pred.shape)} is smaller than {MIN_EXTENT} in some direction (the SSIM window)')
    if not 1 <= len(names) <= ops.VM_MAX_REGIONS:
        raise ValueError(f'score_volume: 1 to {ops.VM_MAX_REGIONS} region names, got {len(names)}')
    pred, gt = pred.float().contiguous(), gt.float().contiguous()
    std = None if std is None else std.float().contiguous()
    _check_finite(pred, gt)
    if std is not None:
        _check_finite(std, None, 'the std volume')
    sums = ops.volume_metrics(pred, gt, region.contiguous(), std, nreg=len(names))
    s2 = metrics.score_device(pred, gt)
    rep = summarize(sums.cpu().numpy(), names, first_plane, has_std=std is not None)
    rep['slice2d'] = {k: (int(s2[k]) if k == 'count' else float(s2[k])) for k in ('psnr', 'ssim', 'mae', 'count', 'global_min', 'global_max')}
    return rep


def score_arrays(pred_vol, gt_raw, label=None, std_vol=None, slice_half_range=80, device='cuda', norm='percentile', more_regions=None):
    """Scores of a prediction as written (host [X, Y, Z] array in [0, 1]) against the raw GT volume, with an optional label volume
    (regions tumor / healthy) and std volume.  `norm`: how the GT is mapped to [-1, 1] (volume.NORMS; the mode the prediction's inputs
    were normalised with).  `more_regions(s0, s1, first_bit)` -> (uint8 [planes, X, Y] bits from first_bit on, their names): further regions
    next to region_mask's (mudiff_hip.known_region: known, synthesised).  -> score_volume's report plus shape and slab [s0, s1], and the
    key norm when it is not the default."""
    from . import ops
    from .volume import normalise_volume
    s0, s1 = check_shapes(np.shape(pred_vol), np.shape(gt_raw), None if label is None else np.shape(label), slice_half_range,
                          None if std_vol is None else np.shape(std_vol))
    device = torch.device(device)
    gt_norm = normalise_volume(gt_raw, norm)
    gt = ops.to_range_0_1(torch.from_numpy(slab_planes(gt_norm, s0, s1)).to(device))
    pred = torch.from_numpy(slab_planes(pred_vol, s0, s1)).to(device)
    std = None if std_vol is None else torch.from_numpy(slab_planes(std_vol, s0, s1)).to(device)
    m, names = region_mask(slab_planes(gt_raw, s0, s1, np.float64), None if label is None else slab_planes(label, s0, s1, np.float64))
    if more_regions is not None:
        bits, more = more_regions(s0, s1, len(names))
        m, names = m | np.asarray(bits, np.uint8), tuple(names) + tuple(more)
    rep = score_volume(pred, gt, torch.from_numpy(m).to(device), std, names, first_plane=s0)
    extra = {} if norm == 'percentile' else dict(norm=norm)
    return dict(shape=[int(v) for v in np.shape(gt_raw)], slab=[s0, s1], **extra, **rep)


def score_files(pred_path, gt_path, mask_path=None, std_path=None, slice_half_range=80, device='cuda', norm='percentile', regrid=False,
                resampled=None, interp='linear'):
    """score_arrays on NIfTI files (volume.read_nifti): the prediction, the raw GT, an optional label volume (--eval_mask, e.g. a
    BraTS segmentation) and an optional std volume.  Warns when the prediction's affine differs from the GT's.  With `regrid`
    (--regrid) a GT or a label volume that is not on the prediction's grid is first resampled onto it (mudiff_hip.volume_regrid:
    trilinear, or a cubic B-spline with interp='cubic' (--regrid_interp) / nearest neighbour); the list `resampled` receives their names."""
    from .volume import read_nifti
    pred, pa, ph = read_nifti(pred_path)
    std = None if std_path is None else read_nifti(std_path)[0]
    done = []
    if regrid:
        from . import volume_intake as VI
        from . import volume_regrid as VR
        gt_raw = VI.read_nifti_raw(gt_path)
        ga = gt_raw.affine
        gt, label, done = VR.eval_onto_grid(pred.shape, VR.world_affine_of(pa, ph), gt_raw,
                                            None if mask_path is None else VI.read_nifti_raw(mask_path), torch.device(device),
                                            names=('gt', 'mask'), interp=interp)
        if resampled is not None:
            resampled.extend(done)
    else:
        gt, ga, _ = read_nifti(gt_path)
        label = None if mask_path is None else read_nifti(mask_path)[0]
    if 'gt' not in done:
        warn_affine(pa, ga, pred_path, gt_path)
    return score_arrays(pred.astype(np.float32), gt, label, None if std is None else std.astype(np.float32), slice_half_range, device,
                        norm=norm)


def eval_inputs_on_grid(ref, gt, label, gt_affine, regrid, half_range, device, names, wording=str, interp='linear', found=None,
                        antialias=False):
    """The evaluation inputs of a prediction on the grid ref = (shape, affine, header) of its first input, checked: under `regrid`
    (--regrid) `gt` and `label` are RawVolumes and what is not on that grid is resampled onto it (volume_regrid.eval_onto_grid, which
    explains `interp`, `found` and `antialias`);
    otherwise they are arrays as volume.read_nifti returns them.  `label` may be None; `gt_affine`: the ground truth's own affine.
    check_shapes' ValueError is raised as ValueError(wording(e)); the affines are compared (warn_affine, with `names` = what to call
    the first input and the ground truth) unless the ground truth was just resampled.  -> ((gt, label), the names of what was resampled)."""
    shape, affine, header = ref
    resampled = []
    if regrid:
        from . import volume_regrid as VR
        gt, label, resampled = VR.eval_onto_grid(shape, VR.world_affine_of(affine, header), gt, label, device, interp=interp, found=found,
                                                  **(dict(antialias=True) if antialias else {}))
    try:
        check_shapes(shape, gt.shape, None if label is None else label.shape, half_range)
    except ValueError as e:
        raise ValueError(wording(e)) from None
    if 'gt_volume' not in resampled:
        warn_affine(affine, gt_affine, *names)
    return (gt, label), resampled


def warn_affine(pred_affine, gt_affine, pred_name='the prediction', gt_name='the ground truth'):
    if np.shape(pred_affine) != np.shape(gt_affine) or not np.allclose(np.asarray(pred_affine), np.asarray(gt_affine)):
        warnings.warn(f'the affines of {pred_name} and {gt_name} differ: the volumes are compared voxel by voxel regardless')


# ---------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(description='Score a predicted volume against its ground truth on the GPU: PSNR, 3D SSIM and MAE per '
                                            'region (slab, brain, and with --mask tumor / healthy), per-plane curves and the 8-bit 2D metrics.')
    p.add_argument('--pred', type=str, required=True, help='predicted volume (NIfTI, values in [0, 1], e.g. predicted_t1ce.nii.gz)')
    p.add_argument('--gt', type=str, required=True, help='raw ground-truth volume (NIfTI); normalised like the pipeline inputs')
    p.add_argument('--mask', type=str, default=None, help='label volume (NIfTI, e.g. a BraTS segmentation): label != 0 is the tumor region')
    p.add_argument('--std', type=str, default=None, help="an ensemble's std volume (predicted_<t>_std.nii.gz): adds the uncertainty block")
    p.add_argument('--slice_half_range', type=int, default=80, help='the slab: the centre +- this many planes (as the volume pipeline)')
    p.add_argument('--norm', type=str, default='percentile', choices=['percentile', 'zscore'],
                   help="how the ground truth is mapped to [-1, 1]: the --norm the prediction was made with (mudiff_hip.volume)")
    p.add_argument('--regrid', action='store_true',
                   help="resample a --gt (trilinearly) or a --mask (nearest neighbour) that is not on the prediction's voxel grid onto "
                        'it through the affines before scoring (mudiff_hip.volume_regrid; resampling, not registration)')
    p.add_argument('--regrid_interp', type=str, default='linear', choices=['linear', 'cubic'],
                   help="how --regrid resamples the --gt: 'linear' = trilinearly; 'cubic' = with a cubic B-spline, which does not soften "
                        'it (mudiff_hip.volume_regrid; the --mask stays nearest neighbour)')
    p.add_argument('--json', type=str, default=None, help='write the full report (per-plane curves included) to this file')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        resampled = []
        rep = score_files(args.pred, args.gt, args.mask, args.std, args.slice_half_range, norm=args.norm, regrid=args.regrid,
                          resampled=resampled, interp=args.regrid_interp)
    except ValueError as e:
        print(f'error: {e}', file=sys.stderr)
        return 2
    if resampled:
        print(f"[metrics] regrid={','.join(resampled)}" + ('' if args.regrid_interp == 'linear' else f' | interp={args.regrid_interp}'))
    for ln in format_lines(rep):
        print(ln)
    if args.json:
        print(f'[metrics] wrote {write_json(rep, args.json)}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
