"""Interval coverage of an ensemble's quantile maps against a ground truth, on the device: does the band between two per-voxel sample
quantiles hold the truth as often as its name says?    volume_metrics' uncertainty block says whether the std is
larger where the error is; this is the other half, the calibration of the band itself.

Definitions (on the slab: the planes s0..s1 that volume.extract_center_slices(z, slice_half_range) selects):
- lo, hi: the fp32 quantile volumes as written (predicted_<t>_q050.nii.gz, predicted_<t>_q950.nii.gz: --ensemble_quantiles, --coverage);
- ground truth: normalised as volume_metrics normalises it (volume.normalise_volume under `norm`, then ops.to_range_0_1);
- regions: volume_metrics.region_mask's (slab, brain = raw GT != 0, and with a label volume tumor and healthy);
- a voxel is `below` when gt < lo, `above` when gt > hi and `inside` otherwise; a voxel where lo, hi or gt is a NaN is `nonfinite` and
  nothing else;
- per region: voxels (all of them), nonfinite, the counts inside_voxels / below_voxels / above_voxels, empirical = inside / (voxels -
  nonfinite) and below, above as the same kind of fraction, mean_width = mean (hi - lo) and mean_width_inside = the same over the inside
  voxels (both in fp64 from the fp32 values), and nominal;
- per_plane: the `empirical` curve of each region over the slab's planes.
A region without finite voxels reports None (null in the JSON) for its fractions and means.

`nominal` is the probability mass between the two SAMPLE quantiles (q_hi - q_lo, as given): with N samples per voxel the band between the
5 % and the 95 % sample quantile is not a 90 % prediction interval (for N = 4 it lies strictly inside the samples' range, which itself
holds a new exchangeable draw with probability 3/5), and no coverage is guaranteed for a finite N.  The number to read `empirical`
against is therefore a convention, not a promise.

The counts and fp64 sums come per plane and region from csrc/volume_coverage.hip (ops.volume_interval_coverage); the totals add them on
the host in plane order, so every number is a fixed function of the inputs.

    python -m mudiff_hip.volume_coverage --lo predicted_t1ce_q050.nii.gz --hi predicted_t1ce_q950.nii.gz --gt t1ce.nii.gz [--mask seg.nii.gz]
                                         [--nominal 0.9] [--norm percentile] [--slice_half_range 80] [--json coverage.json]
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np
import torch


def _ratio(a, b):
    return float(a) / float(b) if b else None


def _block(c, s, nominal):
    """One region's block from its int64 counts (one row of MUD_VC_NC) and fp64 sums (one row of MUD_VC_NS)."""
    from .ops import VC_ABOVE, VC_BELOW, VC_INSIDE, VC_N, VC_NONFINITE, VC_WIDTH, VC_WIDTH_INSIDE
    n, inside, bad = int(c[VC_N]), int(c[VC_INSIDE]), int(c[VC_NONFINITE])
    return dict(voxels=n + bad, nonfinite=bad, inside_voxels=inside, below_voxels=int(c[VC_BELOW]), above_voxels=int(c[VC_ABOVE]),
                empirical=_ratio(inside, n), below=_ratio(c[VC_BELOW], n), above=_ratio(c[VC_ABOVE], n),
                mean_width=_ratio(s[VC_WIDTH], n), mean_width_inside=_ratio(s[VC_WIDTH_INSIDE], inside),
                nominal=None if nominal is None else float(nominal))


def summarize(counts, sums, names, first_plane=0, nominal=None):
    """Per-plane counts (array-like int64 [planes, len(names), MUD_VC_NC]) and sums (fp64 [planes, len(names), MUD_VC_NS];
    ops.volume_interval_coverage) -> dict(regions, coverage {name: block}, per_plane {plane: [...], name: {empirical: [...]}}).  Region
    totals add the planes in plane order (the sums in fp64)."""
    from .ops import VC_NC, VC_NS
    counts, sums = np.asarray(counts, np.int64), np.asarray(sums, np.float64)
    if counts.ndim != 3 or counts.shape[1:] != (len(names), VC_NC) or sums.shape != counts.shape[:2] + (VC_NS,) or counts.shape[0] < 1:
        raise ValueError(f'counts {counts.shape} and sums {sums.shape} are not [planes, {len(names)}, {VC_NC}] and [planes, {len(names)}, {VC_NS}]')
    P = counts.shape[0]
    rep = dict(regions=list(names), coverage={}, per_plane=dict(plane=list(range(int(first_plane), int(first_plane) + P))))
    for k, name in enumerate(names):
        c, s = np.zeros(VC_NC, np.int64), np.zeros(VC_NS, np.float64)
        for z in range(P):
            c, s = c + counts[z, k], s + sums[z, k]
        rep['coverage'][name] = _block(c, s, nominal)
        rep['per_plane'][name] = dict(empirical=[_block(counts[z, k], sums[z, k], nominal)['empirical'] for z in range(P)])
    return rep


def _planes_first(a, dtype):
    return np.ascontiguousarray(np.moveaxis(np.asarray(a), 2, 0), dtype=dtype)


def measure_arrays(lo, hi, gt_raw, label=None, slice_half_range=80, device='cuda', norm='percentile', nominal=None):
    """The coverage of the interval [lo, hi] (host [X, Y, Z] arrays, as written) over the raw ground-truth volume of the same shape, with
    an optional label volume (regions tumor / healthy), on the slab.  `norm`: how the GT is mapped to [-1, 1] (volume.NORMS; the mode
    the prediction's inputs were normalised with); `nominal`: q_hi - q_lo, reported as given.
    -> dict(shape, slab, nominal[, norm], regions, coverage={region: block}, per_plane) (summarize)."""
    from . import ops
    from .volume import normalise_volume
    from .volume_metrics import region_mask, slab_range
    shape = tuple(np.shape(gt_raw))
    if len(shape) != 3:
        raise ValueError(f'the ground truth must be a 3D volume, got shape {shape}')
    for what, a in (('lower quantile volume', lo), ('upper quantile volume', hi), ('label mask', label)):
        if a is not None and tuple(np.shape(a)) != shape:
            raise ValueError(f'the {what} {tuple(np.shape(a))} and the ground truth {shape} differ in shape')
    s0, s1 = slab_range(shape[2], slice_half_range)
    device = torch.device(device)
    m, names = region_mask(_planes_first(gt_raw, np.float64), None if label is None else _planes_first(label, np.float64))
    gt = ops.to_range_0_1(torch.from_numpy(_planes_first(normalise_volume(gt_raw, norm), np.float32)).to(device))
    up = lambda a: torch.from_numpy(_planes_first(a, np.float32)).to(device)      # noqa: E731
    counts, sums, a, _ = ops.volume_interval_coverage(up(lo), up(hi), gt, torch.from_numpy(m).to(device), len(names), s0, s1)
    rep = summarize(counts.cpu().numpy(), sums.cpu().numpy(), names, a, nominal)
    extra = {} if norm == 'percentile' else dict(norm=norm)
    return dict(shape=[int(v) for v in shape], slab=[s0, s1], nominal=None if nominal is None else float(nominal), **extra, **rep)


def measure_files(lo_path, hi_path, gt_path, mask_path=None, slice_half_range=80, device='cuda', norm='percentile', nominal=None):
    """measure_arrays on NIfTI files (volume.read_nifti)."""
    from .volume import read_nifti
    read = lambda path: None if path is None else read_nifti(path)[0]      # noqa: E731
    return measure_arrays(read(lo_path).astype(np.float32), read(hi_path).astype(np.float32), read(gt_path), read(mask_path),
                          slice_half_range, device, norm, nominal)


def _fmt(v, spec='.4f'):
    return 'n/a' if v is None else format(v, spec)


def format_lines(rep):
    """One printed line per region."""
    return [format_line(rep, name) for name in rep['regions']]


def format_line(rep, name):
    """The printed line of one region."""
    c = rep['coverage'][name]
    return (f"[coverage] {name}: empirical {_fmt(c['empirical'])} (nominal {_fmt(c['nominal'], 'g')}) | below {_fmt(c['below'])} | above "
            f"{_fmt(c['above'])} | mean width {_fmt(c['mean_width'], '.6f')} | inside {_fmt(c['mean_width_inside'], '.6f')} | voxels "
            f"{c['voxels']}" + (f" | nonfinite {c['nonfinite']}" if c['nonfinite'] else ''))


def write_json(rep, path):
    with open(path, 'w') as f:
        json.dump(rep, f, indent=1)
    return path


def build_parser():
    p = argparse.ArgumentParser(description="Coverage of an ensemble's quantile interval on the GPU: the share of ground-truth voxels between "
                                            'the lower and the upper quantile volume, per region, with the mean interval width.')
    p.add_argument('--lo', type=str, required=True, help='lower quantile volume (NIfTI, e.g. predicted_t1ce_q050.nii.gz)')
    p.add_argument('--hi', type=str, required=True, help='upper quantile volume (NIfTI, e.g. predicted_t1ce_q950.nii.gz)')
    p.add_argument('--gt', type=str, required=True, help='raw ground-truth volume (NIfTI); normalised like the pipeline inputs')
    p.add_argument('--mask', type=str, default=None, help='label volume (NIfTI, e.g. a BraTS segmentation): label != 0 is the tumor region')
    p.add_argument('--nominal', type=float, default=None,
                   help='the mass between the two sample quantiles (q_hi - q_lo, e.g. 0.9), reported next to the empirical coverage; not a '
                        'guaranteed coverage for a finite number of samples')
    p.add_argument('--norm', type=str, default='percentile', choices=['percentile', 'zscore'],
                   help='how the ground truth is mapped to [-1, 1]: the --norm the prediction was made with (mudiff_hip.volume)')
    p.add_argument('--slice_half_range', type=int, default=80, help='the slab: the centre +- this many planes (as the volume pipeline)')
    p.add_argument('--json', type=str, default=None, help='write the full report (the per-plane curves included) to this file')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        rep = measure_files(args.lo, args.hi, args.gt, args.mask, args.slice_half_range, norm=args.norm, nominal=args.nominal)
    except ValueError as e:
        print(f'error: {e}', file=sys.stderr)
        return 2
    for ln in format_lines(rep):
        print(ln)
    if args.json:
        print(f'[coverage] wrote {write_json(rep, args.json)}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
