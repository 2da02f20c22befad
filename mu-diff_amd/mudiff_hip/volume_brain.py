"""Brain extraction of the inputs (--brain_extract; csrc/volume_brain.hip).

The generators were trained on skull-stripped volumes, and every preparation stage takes a voxel that is exactly 0 for background and
everything else for brain.  --foreground makes that true for the air around a head; the skull and the scalp stay.  With --brain_extract
one mask per subject is estimated from one input, once every input is on the common grid, and applied to all of them before
--bias_correct and the normalisation see them:

    M0 = the tissue mask of volume_foreground (candidates, Otsu bin, mud_volume_fg_mask): shared code, not a copy
    E  = the voxels of M0 farther than erode_mm from the nearest voxel outside M0      (mud_volume_edt(M0, 0), mud_volume_edt_select)
    C  = the largest 6-connected component of E                                        (mud_volume_fg_label(1) / _census / _select)
    B  = the voxels of M0 within dilate_mm of C                                        (mud_volume_edt(C, 1), mud_volume_edt_select)
    plus the holes of B unless --brain_keep_holes                                      (mud_volume_fg_label(0) / _census / _select)

The erosion breaks the thin bridges between brain and scalp, the largest component is the brain's core, and the core grows back inside
the thresholded tissue.  Distances are millimetres on the volume's own (possibly anisotropic) grid: the spacing is the column norms of
its world affine.  This is a classical morphological ESTIMATE of the brain, not a learned extraction: it needs a dark gap (CSF, bone)
between brain and scalp that the erosion radius can open, and its default radii are engineering choices that no brain data was
available to tune.  All per-voxel work is the device's; two runs give the same bits.
"""
from __future__ import annotations

import math
import os

import numpy as np

from . import volume_foreground as VF
from .volume_intake import upload, write_report_json
from .volume_regrid import world_affine_of

MIN_BINS, MAX_BINS = VF.MIN_BINS, VF.MAX_BINS
DEFAULTS = dict(bins=256, erode_mm=5.0, dilate_mm=6.0, keep_holes=False)
SOURCE_PREFERENCE = ('T1', 'T1CE')


def check_options(bins=256, erode_mm=5.0, dilate_mm=6.0, keep_holes=False):
    """ValueError (with the flag's name) for a value the stage cannot run with."""
    if not (float(bins) == int(bins) and MIN_BINS <= int(bins) <= MAX_BINS):
        raise ValueError(f'--brain_bins must be in [{MIN_BINS}, {MAX_BINS}] (got {bins})')
    if not (math.isfinite(float(erode_mm)) and float(erode_mm) > 0):
        raise ValueError(f'--brain_erode_mm must be finite and > 0 (got {erode_mm})')
    if not (math.isfinite(float(dilate_mm)) and float(dilate_mm) >= float(erode_mm)):
        raise ValueError(f'--brain_dilate_mm must be finite and not below --brain_erode_mm = {erode_mm} (got {dilate_mm})')


def spacing_of(vol):
    """(sx, sy, sz) in world units: the column norms of the volume's world affine (volume_regrid.world_affine_of)."""
    lin = np.asarray(world_affine_of(vol.affine, vol.header), np.float64)[:3, :3]
    spacing = tuple(float(np.linalg.norm(lin[:, a])) for a in range(3))
    if not all(math.isfinite(s) and s > 0 for s in spacing):
        raise ValueError(f'brain_mask: the affine gives no voxel spacing (column norms {spacing})')
    return spacing


def source_of(names, brain_from=None):
    """The input the mask is computed from: --brain_from (ValueError when the subject has no such input), else the first of T1, T1CE
    that is among the inputs, else the first input."""
    names = [str(n) for n in names]
    if brain_from is not None:
        if str(brain_from).upper() not in (n.upper() for n in names):
            raise ValueError(f'--brain_from {brain_from} is not among the inputs ({", ".join(names)})')
        return next(n for n in names if n.upper() == str(brain_from).upper())
    for want in SOURCE_PREFERENCE:
        if want in names:
            return want
    return names[0]


def brain_mask(vol, device, bins=256, erode_mm=5.0, dilate_mm=6.0, keep_holes=False):
    """A RawVolume (its voxels on the host, or on the device already) -> (device uint8 mask [Z,Y,X] or None, report).  report:
    threshold, bin, bins, lo, hi, candidates (as volume_foreground's), spacing, erode_mm, dilate_mm, tissue (|M0|), eroded (|E|),
    components (of E), core (|C|), kept (mask voxels), filled (of them, added as holes), source (None: the caller's to fill in).
    None - leave the inputs as they are - without a candidate, with hi == lo, with fewer than two non-empty bins or when the erosion
    leaves nothing."""
    from . import ops
    if len(vol.shape) != 3:
        raise ValueError(f'brain_mask: expected a 3D volume, got shape {tuple(vol.shape)}')
    check_options(bins, erode_mm, dilate_mm, keep_holes)
    bins, erode_mm, dilate_mm = int(bins), float(erode_mm), float(dilate_mm)
    spacing = spacing_of(vol)
    dev, meta = upload(vol, device), vol.kernel_meta('foreground')
    shape = meta[1]
    report = dict(threshold=None, bin=None, bins=bins, lo=None, hi=None, candidates=0, spacing=list(spacing), erode_mm=erode_mm,
                  dilate_mm=dilate_mm, tissue=0, eroded=0, components=0, core=0, kept=0, filled=0, source=None)
    tissue = VF.threshold_mask(dev, meta, bins, report)
    if tissue is None:
        return None, report
    d2 = ops.volume_edt(tissue, shape, 0, spacing)
    report['tissue'] = int(VF._word(ops.volume_edt_select(d2, 0.0, True)[1])[0])      # (d2 > 0 exactly on M0: a radius of 0 counts it)
    eroded, count = ops.volume_edt_select(d2, erode_mm * erode_mm, True)
    report['eroded'] = int(VF._word(count)[0])
    if report['eroded'] == 0:
        return None, report
    core, report['core'], report['components'] = VF.largest_component(eroded, shape)
    mask, count = ops.volume_edt_select(ops.volume_edt(core, shape, 1, spacing), dilate_mm * dilate_mm, False, tissue)
    report['kept'] = int(VF._word(count)[0])
    if not keep_holes:
        mask, report['filled'] = VF.fill_holes(mask, shape)
        report['kept'] += report['filled']
    return mask, report


def apply_mask(vol, mask, device):
    """The volume with every voxel outside the device mask set to exactly 0: a MaskedVolume with the volume's own geometry."""
    from . import ops
    out = ops.volume_fg_apply(upload(vol, device), *vol.kernel_meta('foreground'), mask)[0]
    return VF.MaskedVolume(out, vol.shape, vol.affine, vol.header)


def host_mask(mask):
    """A device mask [Z,Y,X] -> uint8 [X,Y,Z] on the host, in file order."""
    return np.asfortranarray(mask.cpu().numpy().transpose(2, 1, 0))


# ---------------------------------------------------------------------------------------------------
# the pipeline's side
# ---------------------------------------------------------------------------------------------------
def add_flags(p):
    p.add_argument('--brain_extract', action='store_true',
                   help='estimate one brain mask per subject and set the voxels of every input outside it to exactly 0, once the inputs '
                        'are on the common grid (after --coregister / --regrid) and before --bias_correct and the normalisation see '
                        'them: the tissue mask of --foreground, eroded by --brain_erode_mm so that the bridges between brain and scalp '
                        'break, its largest component grown back by --brain_dilate_mm inside the tissue, holes filled (exact Euclidean '
                        'distance transform with the voxel spacing, on the GPU: mudiff_hip.volume_brain); brain_<t>.json next to the '
                        'prediction holds what was found.  This is a morphological estimate, not a learned brain extraction.  '
                        '--gt_volume / --eval_mask are not masked')
    p.add_argument('--brain_from', type=str, default=None,
                   help='the input the mask is estimated from (T1, T1CE, T2 or FLAIR; default: T1, else T1CE, else the first input)')
    p.add_argument('--brain_erode_mm', type=float, default=DEFAULTS['erode_mm'], help='erosion radius in millimetres (finite, > 0)')
    p.add_argument('--brain_dilate_mm', type=float, default=DEFAULTS['dilate_mm'],
                   help='how far the eroded core grows back, in millimetres, inside the thresholded tissue (not below --brain_erode_mm)')
    p.add_argument('--brain_bins', type=int, default=DEFAULTS['bins'], help='bins of the histogram the Otsu threshold is taken from (16 to 1024)')
    p.add_argument('--brain_keep_holes', action='store_true', help='with --brain_extract: do not fill the holes of the mask')
    p.add_argument('--brain_mask_out', action='store_true',
                   help='with --brain_extract: also write brain_<t>_mask.nii.gz, the uint8 mask on the grid of the first input')


def options_from(args):
    """A namespace's --brain_* flags (any may be missing) -> IntakeOptions' `brain`: the keyword arguments of brain_mask plus `source`
    (--brain_from or None) and `mask_out`, or None without --brain_extract.  ValueError, naming the flag, for a value check_options refuses."""
    kw = {k: getattr(args, 'brain_' + k, v) for k, v in DEFAULTS.items()}
    check_options(**kw)
    source = getattr(args, 'brain_from', None)
    kw = dict({k: type(v)(kw[k]) for k, v in DEFAULTS.items()}, source=None if source is None else str(source),
              mask_out=bool(getattr(args, 'brain_mask_out', False)))
    return dict(brain=kw if getattr(args, 'brain_extract', False) else None)


def brain_suffix(reports):
    """What a [done] line gains under --brain_extract (nothing otherwise): ` | brain=<source>`."""
    if not reports:
        return ''
    return ' | brain=' + ','.join(str(r[0]) for r in reports)


def write_reports(reports, output_dir, target, affine=None, header=None):
    """brain_<t>.json next to the prediction: the report of the subject's mask; with --brain_mask_out also brain_<t>_mask.nii.gz, the
    uint8 mask on the common grid (affine / header: that grid's).  reports: [(source name, report, host mask or None)].  -> the json's
    path."""
    path = write_report_json('brain', reports[0][1], output_dir, target)
    mask = reports[0][2] if len(reports[0]) > 2 else None
    if mask is not None:
        VF.write_mask(os.path.join(output_dir, f'brain_{target.lower()}_mask.nii.gz'), mask, np.eye(4) if affine is None else affine, header)
    return path
