"""Foreground masking of the inputs (--foreground; csrc/volume_foreground.hip).

The volume pipeline takes a voxel that is exactly 0 for background and everything else for brain: the percentiles and the z-score moments,
the log image of --bias_correct and the pass-through rule of --denoise all rest on it.  A head that was never masked (Rician air around
it), a stripped volume with small non-zero values outside, a detached bright artefact break that rule.  With --foreground every input is
replaced by itself with the voxels outside its foreground mask set to exactly 0, on its own grid, before --coregister / --regrid /
--bias_correct see it:

    stored voxels --mud_volume_fg_range / _hist--> counts of the candidates (finite, != 0) --otsu_bin, on the host--> the threshold bin
    mud_volume_fg_mask --> uint8 mask; --foreground_open N: N erosions, then N dilations (mud_volume_fg_morph)
    mud_volume_fg_label(1) / _census / _select --> the largest 6-connected component
    mud_volume_fg_label(0) / _census / _select --> plus its holes (the components of the complement that touch no face)
    mud_volume_fg_apply --> fp32 [Z,Y,X], a volume like a regridded one, with the source's own geometry

This is a foreground (head or object) mask by thresholding and topology.  It is not a brain extraction: the skull and the scalp stay
(--brain_extract, mudiff_hip.volume_brain, estimates the brain by morphology on top of the same threshold).
All per-voxel work is the device's and all of it is integer work: the host sees the counts and a few words per stage, and two runs give
the same bits.
"""
from __future__ import annotations

import os

import numpy as np

from . import MudiffHipError
from .volume_intake import upload, write_report_json
from .volume_regrid import RegriddedVolume

MIN_BINS, MAX_BINS, MAX_OPEN = 16, 1024, 3
DEFAULTS = dict(bins=256, open=0, keep_holes=False, mask_out=False)


class MaskedVolume(RegriddedVolume):
    """A RawVolume whose voxels live on the device (fp32 [Z,Y,X]) with the shape, affine and header of the volume it was made from.
    `mask`: the uint8 [X,Y,Z] foreground mask on the host under --foreground_mask_out, else None."""
    mask = None


def check_options(bins=256, open=0, keep_holes=False, mask_out=False):      # noqa: A002  (`open` is the flag's name)
    """ValueError (with the flag's name) for a value the kernels cannot run with."""
    if not (float(bins) == int(bins) and MIN_BINS <= int(bins) <= MAX_BINS):
        raise ValueError(f'--foreground_bins must be in [{MIN_BINS}, {MAX_BINS}] (got {bins})')
    if not (float(open) == int(open) and 0 <= int(open) <= MAX_OPEN):
        raise ValueError(f'--foreground_open must be in [0, {MAX_OPEN}] (got {open})')


def otsu_bin(counts):
    """Otsu's threshold bin of integer counts, in fp64 and in index order: over k = 0 .. bins - 2 with a = sum_{i<=k} c_i and b = n - a both
    > 0, s_k = a * b * (m0 / a - (mt - m0) / b)^2 with m0 = sum_{i<=k} i c_i and mt the same over all bins; the first k with the
    largest s_k.  None when fewer than two bins are non-empty."""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    if any(v < 0 for v in c):
        raise MudiffHipError('otsu_bin: negative counts')
    if sum(1 for v in c if v) < 2:
        return None
    n = sum(c)
    mt = float(sum(i * v for i, v in enumerate(c)))
    a = m0 = 0
    best, best_s = None, -1.0
    for k in range(len(c) - 1):
        a += c[k]
        m0 += k * c[k]
        b = n - a
        if a == 0 or b == 0:
            continue
        d = float(m0) / float(a) - (mt - float(m0)) / float(b)
        s = float(a) * float(b) * (d * d)
        if s > best_s:
            best, best_s = k, s
    return best


def unkey(key):
    """The fp32 behind an order-preserving key of mud_volume_fg_range (bits | 0x80000000 for v >= 0, ~bits for v < 0)."""
    key = int(key) & 0xFFFFFFFF
    bits = key ^ 0x80000000 if key & 0x80000000 else ~key & 0xFFFFFFFF
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def _word(t, dtype=np.uint32):
    return t.cpu().numpy().view(dtype)


def threshold_mask(dev, meta, bins, report):
    """The first half of foreground(), shared with volume_brain.brain_mask: the candidates' range and histogram, the Otsu bin and the
    raw mask (device uint8 [Z,Y,X]) of the candidates above it.  Fills report's candidates, lo, hi, bin and threshold as far as it gets;
    None without a candidate, with hi == lo or with fewer than two non-empty bins."""
    from . import ops
    found = _word(ops.volume_fg_range(dev, *meta))
    report['candidates'] = int(found[2])
    if report['candidates'] == 0:
        return None
    lo, hi = unkey(~int(found[0])), unkey(found[1])
    report['lo'], report['hi'] = lo, hi
    if hi == lo:
        return None
    scale = bins / (hi - lo)
    k = otsu_bin(_word(ops.volume_fg_hist(dev, *meta, lo, scale, bins)).astype(np.int64))
    if k is None:
        return None
    report['bin'], report['threshold'] = k, lo + (k + 1) / scale
    return ops.volume_fg_mask(dev, *meta, lo, scale, bins, k)


def largest_component(mask, shape):
    """-> (the largest 6-connected component of a device mask, or None for an empty mask; its voxels; the number of components)."""
    from . import ops
    labels = ops.volume_fg_label(mask, shape, 1)
    winner, components = (int(v) for v in _word(ops.volume_fg_census(labels, shape)[1], np.uint64))
    if not components:
        return None, 0, 0
    return ops.volume_fg_select(labels, None, 0xFFFFFFFF - (winner & 0xFFFFFFFF), False)[0], winner >> 32, components


def fill_holes(mask, shape):
    """Switches on, in `mask` itself, the components of its complement that touch no face of the volume -> (mask, the voxels added)."""
    from . import ops
    labels = ops.volume_fg_label(mask, shape, 0)
    mask, filled = ops.volume_fg_select(labels, ops.volume_fg_census(labels, shape)[0], 0, True, mask)
    return mask, int(_word(filled)[0])


def foreground(raw, device, bins=256, open=0, keep_holes=False, mask_out=False):      # noqa: A002
    """A RawVolume (its voxels on the host, or on the device already) -> (MaskedVolume, report).  report: threshold (fp64, for
    information: the bin is what is compared), bin, bins, lo, hi, candidates, components (of the mask the largest one was taken from),
    kept (mask voxels), filled (of them, added as holes), removed (candidates set to 0), open, keep_holes.  Without a candidate, with
    hi == lo or with fewer than two non-empty bins the input itself is returned and the report holds threshold None."""
    from . import ops
    if len(raw.shape) != 3:
        raise ValueError(f'foreground: expected a 3D volume, got shape {tuple(raw.shape)}')
    check_options(bins, open, keep_holes, mask_out)
    bins, steps = int(bins), int(open)
    dev, meta = upload(raw, device), raw.kernel_meta('foreground')
    shape = meta[1]
    report = dict(threshold=None, bin=None, bins=bins, lo=None, hi=None, candidates=0, components=0, kept=0, filled=0, removed=0,
                  open=steps, keep_holes=bool(keep_holes))
    mask = threshold_mask(dev, meta, bins, report)
    if mask is None:
        return raw, report
    for dilate in (False,) * steps + (True,) * steps:
        mask = ops.volume_fg_morph(mask, shape, dilate)
    kept, report['kept'], report['components'] = largest_component(mask, shape)
    if kept is not None:
        mask = kept
        if not keep_holes:
            mask, report['filled'] = fill_holes(mask, shape)
            report['kept'] += report['filled']
    out, removed = ops.volume_fg_apply(dev, *meta, mask)      # (an opening that left nothing: every candidate goes)
    report['removed'] = int(_word(removed)[0])
    vol = MaskedVolume(out, raw.shape, raw.affine, raw.header)
    if mask_out:
        vol.mask = np.asfortranarray(mask.cpu().numpy().transpose(2, 1, 0))
    return vol, report


# ---------------------------------------------------------------------------------------------------
# the pipeline's side
# ---------------------------------------------------------------------------------------------------
def add_flags(p):
    p.add_argument('--foreground', action='store_true',
                   help='set the voxels outside a foreground mask of every input to exactly 0, on its own grid, after --denoise and before '
                        '--coregister / --regrid / --bias_correct see it (Otsu threshold, largest 6-connected component, holes filled, on '
                        'the GPU: mudiff_hip.volume_foreground); foreground_<t>.json next to the prediction holds what was found.  This is '
                        'a head / object mask by thresholding and topology, NOT a brain extraction: the skull stays (see --brain_extract).  '
                        '--gt_volume / --eval_mask are not masked')
    p.add_argument('--foreground_bins', type=int, default=DEFAULTS['bins'], help='bins of the histogram the Otsu threshold is taken from (16 to 1024)')
    p.add_argument('--foreground_open', type=int, default=DEFAULTS['open'],
                   help='open the thresholded mask first: this many erosions, then as many dilations, over the 6-neighbourhood (0 to 3)')
    p.add_argument('--foreground_keep_holes', action='store_true', help='with --foreground: do not fill the holes of the kept component')
    p.add_argument('--foreground_mask_out', action='store_true',
                   help='with --foreground: also write foreground_<t>_<name>.nii.gz, the uint8 mask of each input on its own grid')


def options_from(args):
    """A namespace's --foreground_* flags (any may be missing) -> IntakeOptions' `foreground`: the keyword arguments of foreground, or
    None without --foreground.  ValueError, naming the flag, for a value check_options refuses."""
    kw = {k: getattr(args, 'foreground_' + k, v) for k, v in DEFAULTS.items()}
    check_options(**kw)
    return dict(foreground={k: type(v)(kw[k]) for k, v in DEFAULTS.items()} if getattr(args, 'foreground', False) else None)


def foreground_suffix(reports):
    """What a [done] line gains under --foreground (nothing otherwise): ` | foreground=<name>,<name>,...`."""
    if not reports:
        return ''
    return ' | foreground=' + ','.join(str(r[0]) for r in reports)


def write_mask(path, mask, affine, header=None):
    """A uint8 [X,Y,Z] mask with a volume's geometry -> .nii / .nii.gz (datatype 2)."""
    from .volume import write_nifti1
    mask = np.asarray(mask, dtype=np.uint8)
    try:
        import nibabel as nib
        nib.save(nib.Nifti1Image(mask, affine), path)
        return
    except ImportError:
        pass
    write_nifti1(path, mask, affine, header, 2, 8)


def write_reports(reports, output_dir, target, affine=None, header=None):
    """foreground_<t>.json next to the prediction: {input name: report}; with --foreground_mask_out also foreground_<t>_<name>.nii.gz,
    each input's uint8 mask on that input's own grid.  reports: [(name, report, masked volume or None)]; affine / header: the geometry
    for a mask whose volume carries none.  -> the json's path."""
    path = write_report_json('foreground', {r[0]: r[1] for r in reports}, output_dir, target)
    for r in reports:
        vol = r[2] if len(r) > 2 else None
        if vol is not None and getattr(vol, 'mask', None) is not None:
            own = vol.affine if vol.affine is not None else (np.eye(4) if affine is None else affine)
            write_mask(os.path.join(output_dir, f'foreground_{target.lower()}_{str(r[0]).lower()}.nii.gz'), vol.mask, own,
                       vol.header if vol.header is not None else header)
    return path
