"""Through-plane roughness of a predicted volume, on the device: the number that isolates the stripes of slice-wise synthesis
(DESIGN.md section 5.23).  It needs no ground truth; with one, the same numbers are reported for it, so that a prediction can be read
against what an anatomy of that kind looks like.

Definitions (on the slab: the planes s0..s1 that volume.extract_center_slices(z, slice_half_range) selects; V the fp32 values; a voxel
is `inside` when the mask is non-zero there - by default every slab voxel, or with a ground truth the voxels where the raw GT != 0):
- mean_dz  = mean |V[k+1] - V[k]| over the voxel pairs of neighbouring planes that are both inside;
- mean_dzz = mean |V[k+1] - 2 V[k] + V[k-1]| over the triples that are all inside;
- mean_dx, mean_dy: the same first differences along the two in-plane axes;
- anisotropy = mean_dz / ((mean_dx + mean_dy) / 2): 1 for a volume as smooth across planes as within them;
- dz[k]: the per-plane-pair curve of mean_dz (pair (k, k+1) is listed under k, for k = s0..s1-1).
A mean without pairs is None (null in the JSON), and so is an anisotropy without all three means or with flat planes.

The fp64 sums of fp64 differences come per plane from csrc/volume_through_plane.hip (ops.volume_through_plane); the totals add them on
the host in plane order, so every number is a fixed function of the inputs.  Voxel sizes are not used: a volume with thick slices has
an anisotropy above 1 for that reason alone, which is why the ground truth's own number is reported next to the prediction's.

    python -m mudiff_hip.volume_through_plane --pred predicted_t1ce.nii.gz [--gt t1ce.nii.gz] [--mask seg.nii.gz] [--slice_half_range 80]
                                              [--json through_plane.json]
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np
import torch


def _mean(s, n):
    return float(s) / float(n) if n else None


def summarize(sums, first_plane=0):
    """Per-plane sums (array-like [planes, MUD_TP_NQ], fp64; ops.volume_through_plane) -> dict(mean_dz, mean_dzz, mean_dx, mean_dy,
    anisotropy, pairs_dz, triples_dzz, pairs_dx, pairs_dy, planes=[first, last], dz=[...]).  Totals add the planes in plane order (fp64)."""
    from .ops import TP_N_DX, TP_N_DY, TP_N_DZ, TP_N_DZZ, TP_NQ, TP_S_DX, TP_S_DY, TP_S_DZ, TP_S_DZZ
    sums = np.asarray(sums, np.float64)
    if sums.ndim != 2 or sums.shape[1] != TP_NQ or sums.shape[0] < 1:
        raise ValueError(f'sums of shape {sums.shape} are not [planes, {TP_NQ}]')
    P = sums.shape[0]
    tot = np.zeros(TP_NQ, np.float64)
    for z in range(P):
        tot = tot + sums[z]
    m = dict(mean_dz=_mean(tot[TP_S_DZ], tot[TP_N_DZ]), mean_dzz=_mean(tot[TP_S_DZZ], tot[TP_N_DZZ]), mean_dx=_mean(tot[TP_S_DX], tot[TP_N_DX]),
             mean_dy=_mean(tot[TP_S_DY], tot[TP_N_DY]))
    inplane = None if m['mean_dx'] is None or m['mean_dy'] is None else (m['mean_dx'] + m['mean_dy']) / 2.0
    m['anisotropy'] = m['mean_dz'] / inplane if m['mean_dz'] is not None and inplane else None
    m.update(pairs_dz=int(tot[TP_N_DZ]), triples_dzz=int(tot[TP_N_DZZ]), pairs_dx=int(tot[TP_N_DX]), pairs_dy=int(tot[TP_N_DY]),
             planes=[int(first_plane), int(first_plane) + P - 1], dz=[_mean(sums[z, TP_S_DZ], sums[z, TP_N_DZ]) for z in range(P - 1)])
    return m


def measure_volume(vol, mask=None, z0=0, z1=None):
    """The measure of a device tensor [Z, X, Y] (fp32, planes contiguous) over the planes z0..z1 clipped to it, with an optional uint8
    mask of its shape (non-zero: inside) -> summarize's dict."""
    from . import ops
    sums, a, _ = ops.volume_through_plane(vol.float(), mask, z0, z1)
    return summarize(sums.cpu().numpy(), a)


def _planes_first(a, dtype):
    return np.ascontiguousarray(np.moveaxis(np.asarray(a), 2, 0), dtype=dtype)


def measure_arrays(pred_vol, gt_raw=None, mask=None, slice_half_range=80, device='cuda', norm='percentile'):
    """The measure of a prediction as written (host [X, Y, Z] array) on its slab, and with `gt_raw` (the raw ground-truth volume of the
    same shape) of the ground truth normalised as volume_metrics does it (volume.normalise_volume under `norm`, then ops.to_range_0_1).
    `mask`: a volume of the same shape, non-zero = inside; by default every voxel, or with a ground truth the voxels where it is not 0.
    -> dict(shape, slab, mask, prediction={...}[, ground_truth={...}, dz_ratio])."""
    from . import ops
    from .volume import normalise_volume
    from .volume_metrics import slab_range
    shape = tuple(np.shape(pred_vol))
    if len(shape) != 3:
        raise ValueError(f'the prediction must be a 3D volume, got shape {shape}')
    for what, a in (('ground truth', gt_raw), ('mask', mask)):
        if a is not None and tuple(np.shape(a)) != shape:
            raise ValueError(f'the {what} {tuple(np.shape(a))} and the prediction {shape} differ in shape')
    s0, s1 = slab_range(shape[2], slice_half_range)
    device = torch.device(device)
    inside, which = None, 'slab'
    if mask is not None:
        inside, which = np.asarray(mask) != 0, 'mask'
    elif gt_raw is not None:
        inside, which = np.asarray(gt_raw) != 0, 'gt != 0'
    m = None if inside is None else torch.from_numpy(_planes_first(inside, np.uint8)).to(device)
    rep = dict(shape=[int(v) for v in shape], slab=[s0, s1], mask=which, **({} if norm == 'percentile' else dict(norm=norm)))
    rep['prediction'] = measure_volume(torch.from_numpy(_planes_first(pred_vol, np.float32)).to(device), m, s0, s1)
    if gt_raw is not None:
        gt = ops.to_range_0_1(torch.from_numpy(_planes_first(normalise_volume(gt_raw, norm), np.float32)).to(device))
        rep['ground_truth'] = measure_volume(gt, m, s0, s1)
        p, g = rep['prediction']['mean_dz'], rep['ground_truth']['mean_dz']
        rep['dz_ratio'] = p / g if p is not None and g else None
    return rep


def measure_files(pred_path, gt_path=None, mask_path=None, slice_half_range=80, device='cuda', norm='percentile'):
    """measure_arrays on NIfTI files (volume.read_nifti)."""
    from .volume import read_nifti
    read = lambda path: None if path is None else read_nifti(path)[0]      # noqa: E731
    return measure_arrays(read(pred_path).astype(np.float32), read(gt_path), read(mask_path), slice_half_range, device, norm)


def _fmt(v, spec='.6f'):
    return 'n/a' if v is None else format(v, spec)


def format_line(rep):
    """The one printed line."""
    p = rep['prediction']
    line = (f"[through-plane] slab {rep['slab'][0]}..{rep['slab'][1]} ({rep['mask']}): mean|dz| {_fmt(p['mean_dz'])} | mean|dzz| {_fmt(p['mean_dzz'])} | "
            f"mean|dx| {_fmt(p['mean_dx'])} | mean|dy| {_fmt(p['mean_dy'])} | anisotropy {_fmt(p['anisotropy'], '.4f')}")
    g = rep.get('ground_truth')
    if g is not None:
        line += f" | gt mean|dz| {_fmt(g['mean_dz'])} anisotropy {_fmt(g['anisotropy'], '.4f')} | dz ratio {_fmt(rep['dz_ratio'], '.4f')}"
    return line


def write_json(rep, path):
    with open(path, 'w') as f:
        json.dump(rep, f, indent=1)
    return path


def build_parser():
    p = argparse.ArgumentParser(description='Through-plane roughness of a predicted volume on the GPU: mean |dV/dz|, |d2V/dz2|, the in-plane '
                                            'analogues, their ratio and the per-plane-pair curve over the slab.')
    p.add_argument('--pred', type=str, required=True, help='predicted volume (NIfTI, e.g. predicted_t1ce.nii.gz)')
    p.add_argument('--gt', type=str, default=None,
                   help='raw ground-truth volume (NIfTI): the same numbers for it, normalised like the pipeline inputs; the mask is then GT != 0')
    p.add_argument('--mask', type=str, default=None, help='mask volume (NIfTI): non-zero voxels are measured (default: GT != 0, else every voxel)')
    p.add_argument('--slice_half_range', type=int, default=80, help='the slab: the centre +- this many planes (as the volume pipeline)')
    p.add_argument('--norm', type=str, default='percentile', choices=['percentile', 'zscore'], help='how --gt is mapped to [-1, 1] (mudiff_hip.volume)')
    p.add_argument('--json', type=str, default=None, help='write the full report (the dz curve included) to this file')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        rep = measure_files(args.pred, args.gt, args.mask, args.slice_half_range, norm=args.norm)
    except ValueError as e:
        print(f'error: {e}', file=sys.stderr)
        return 2
    print(format_line(rep))
    if args.json:
        print(f'[through-plane] wrote {write_json(rep, args.json)}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
