"""Inputs conformed to the training grid (--conform, --antialias; csrc/volume_lowpass.hip: mud_volume_lowpass).

The checkpoints were trained on BraTS: 240 x 240 x 155 voxels of 1 mm, axis-aligned, stored LPS.  The volume pipeline takes the first
input's storage grid as it is, so a 0.45 mm acquisition, a 256 mm field of view or a tilted stack reach the generators at a scale, with
a slab and along planes they never saw.  With --conform every input, the first included, is resampled once onto one axis-aligned grid
of the training geometry, placed in the first input's world:

    conform_grid(first shape, first world affine)  -->  (shape, affine): +-spacing per axis by the orientation code, the grid centre on
                                                        the world position of the first input's own grid centre
    stored voxels --upload--> [mud_volume_lowpass] --> mud_volume_regrid / _cubic (inv(source affine) @ [W @] grid affine) --> fp32 [Z,Y,X]

The resamplers are point samplers: where the target grid is coarser than the source they read one neighbourhood per target voxel and
skip the rest, which keeps the noise at full amplitude and folds fine structure into the result.  The low-pass in front of them
(--antialias, on under --conform) is a separable Gaussian per SOURCE axis a: with M = volume_regrid.grid_matrix (reference index ->
source coordinate), f_a = |row a of M's 3 x 3 part| is the number of source voxels one reference step covers along a, and

    sigma_a = sqrt(f_a^2 - 1) / (2 sqrt(2 ln 2)) source voxels for f_a > 1, else exactly 0;   R_a = ceil(3 sigma_a)

the Gaussian whose FWHM, added in quadrature to the source voxel, gives the target voxel.  This rule is an untuned default, not a
measured optimum.  A factor within F_ONE_TOL of 1 is 1: affines come from fp32 headers and through an fp64 solve, and a rotation must
not filter.  The weights are computed here, in fp64, and handed to the kernel; a pass with sigma 0 is skipped, and with all three
skipped nothing is launched and the stored voxels are resampled exactly as without the flag.

Definitions (numpy only, no device): conform_grid, conformed_header, factors, sigmas, radius, weights, lowpass_plan, entry,
conform_suffix, antialias_suffix, write_reports.  On the device: lowpass (ops.volume_lowpass), write_back (volume_regrid.regrid_to).
"""
from __future__ import annotations

import math
import os
import struct

import numpy as np

from .volume_intake import write_report_json
from .volume_reorient import DEFAULT_TARGET, NEGATIVE, POSITIVE, check_target, obliquity_deg

DEFAULT_SHAPE = (240, 240, 155)                          # BraTS
DEFAULT_SPACING = (1.0, 1.0, 1.0)
FWHM_PER_SIGMA = 2.0 * math.sqrt(2.0 * math.log(2.0))
F_ONE_TOL = 1e-6                                         # a sampling factor this close to 1 is 1 (fp32 affines: ~1e-7 relative)
MAX_RADIUS = 16                                          # mud_volume_lowpass's limit: factors up to ~12.5


def _shape3(shape, what='shape'):
    s = tuple(int(v) for v in shape)
    if len(s) != 3 or min(s) < 1:
        raise ValueError(f'conform: {what} must be three positive integers, got {tuple(shape)}')
    return s


def _spacing3(spacing):
    s = [float(v) for v in (spacing if np.ndim(spacing) else [spacing])]
    if len(s) == 1:
        s = s * 3
    if len(s) != 3 or not all(np.isfinite(v) and v > 0 for v in s):
        raise ValueError(f'conform: the spacing must be one or three positive finite values in mm, got {spacing}')
    return tuple(s)


def conform_grid(first_shape, first_world_affine, shape=DEFAULT_SHAPE, spacing=DEFAULT_SPACING, target=DEFAULT_TARGET):
    """The conform grid of a first input of `first_shape` whose voxel -> world matrix is `first_world_affine` (4 x 4) -> (shape, affine).
    Voxel axis v of the grid runs towards letter v of `target` (volume_reorient.check_target: any of the 48 codes) in steps of
    spacing[v]: the 3 x 3 part has +-spacing[v] in column v, in the row of that letter's world axis, and zeros elsewhere (for 'LPS':
    diag(-sx, -sy, +sz)).  The translation puts the grid centre ((X-1)/2, (Y-1)/2, (Z-1)/2) on the world position of the first input's own
    grid centre.  All fp64.  Axis-aligned by construction: an oblique first input is de-obliqued."""
    target = check_target(target)
    shape, spacing, first_shape = _shape3(shape), _spacing3(spacing), _shape3(first_shape, 'the first input\'s shape')
    a = np.asarray(first_world_affine, np.float64)
    if a.shape != (4, 4) or not np.isfinite(a).all():
        raise ValueError(f'conform: need a finite 4 x 4 affine, got {a.tolist() if a.size <= 16 else a.shape}')
    out = np.zeros((4, 4), np.float64)
    for v, letter in enumerate(target):
        w = POSITIVE.index(letter) if letter in POSITIVE else NEGATIVE.index(letter)
        out[w, v] = spacing[v] if letter in POSITIVE else -spacing[v]
    centre = a[:3, :3] @ ((np.asarray(first_shape, np.float64) - 1.0) / 2.0) + a[:3, 3]
    out[:3, 3] = centre - out[:3, :3] @ ((np.asarray(shape, np.float64) - 1.0) / 2.0)
    out[3, 3] = 1.0
    return shape, out


def conformed_header(shape, affine, like=None):
    """The little-endian 348-byte NiftiHeader of a volume on the conform grid: dim and pixdim[1..3] from the grid, datatype F4 (bitpix 32,
    vox_offset 352), scl_slope 1, scl_inter 0, the sform rows set to `affine`, sform_code 1, qform_code 0.  Everything else is copied from
    `like` (the first input's header) when that is a little-endian NiftiHeader; of a big-endian one the text fields (db_name, descrip,
    aux_file, intent_name) and xyzt_units are copied; any other `like` (None, a nibabel header) gives a blank rest.  volume.write_nifti
    reuses the result as it reuses any header."""
    from .volume import NiftiHeader
    shape, a = _shape3(shape), np.asarray(affine, np.float64)
    raw = bytearray(348)
    if isinstance(like, NiftiHeader):
        if like.endian == '<':
            raw = bytearray(like.raw)
        else:
            for lo, hi in ((14, 32), (123, 124), (148, 228), (228, 252), (328, 344)):
                raw[lo:hi] = like.raw[lo:hi]
    pix = list(struct.unpack_from('<8f', raw, 76))
    if not np.isfinite(pix[0]) or pix[0] == 0:
        pix[0] = 1.0
    pix[1:4] = [float(np.sqrt((a[:3, v] ** 2).sum())) for v in range(3)]
    pix[4:] = [p if np.isfinite(p) else 0.0 for p in pix[4:]]
    struct.pack_into('<i', raw, 0, 348)
    struct.pack_into('<8h', raw, 40, 3, *shape, 1, 1, 1, 1)
    struct.pack_into('<h', raw, 70, 16)
    struct.pack_into('<h', raw, 72, 32)
    struct.pack_into('<8f', raw, 76, *pix)
    struct.pack_into('<f', raw, 108, 352.0)
    struct.pack_into('<2f', raw, 112, 1.0, 0.0)
    struct.pack_into('<h', raw, 252, 0)
    struct.pack_into('<h', raw, 254, 1)
    for r in range(3):
        struct.pack_into('<4f', raw, 280 + 16 * r, *[float(v) for v in a[r]])
    raw[344:348] = b'n+1\0'
    return NiftiHeader(bytes(raw), '<')


# ---------------------------------------------------------------------------------------------------
# the anti-aliasing rule
# ---------------------------------------------------------------------------------------------------
def factors(M):
    """Per SOURCE axis a the Euclidean norm of row a of the 3 x 3 part of the sampling matrix M (volume_regrid.grid_matrix): the source
    voxels along a that one step on the reference grid covers.  The spacing ratio for axis-aligned grids; 1 for a rotation."""
    lin = np.asarray(M, np.float64)[:3, :3]
    return [float(np.sqrt((lin[a] * lin[a]).sum())) for a in range(3)]


def sigma_of(f):
    """sqrt(f^2 - 1) / (2 sqrt(2 ln 2)) source voxels for a factor above 1 (by more than F_ONE_TOL), else exactly 0."""
    f = float(f)
    return math.sqrt(f * f - 1.0) / FWHM_PER_SIGMA if f > 1.0 + F_ONE_TOL else 0.0


def sigmas(M):
    return [sigma_of(f) for f in factors(M)]


def radius(sigma):
    return int(math.ceil(3.0 * float(sigma)))


def weights(sigma):
    """w[t + R] = exp(-t^2 / (2 sigma^2)), t = -R..R, R = ceil(3 sigma), in fp64; None for sigma 0 (the pass is skipped)."""
    sigma = float(sigma)
    if sigma == 0.0:
        return None
    t = np.arange(-radius(sigma), radius(sigma) + 1, dtype=np.float64)
    return np.exp(-(t * t) / (2.0 * sigma * sigma))


def lowpass_plan(M, name='the volume'):
    """-> dict(factors, sigmas, radii, weights): per source axis; weights[a] is None where nothing is filtered.  ValueError, naming the
    input and the axis, for a radius above MAX_RADIUS."""
    f = factors(M)
    s = [sigma_of(v) for v in f]
    r = [radius(v) for v in s]
    for a in range(3):
        if r[a] > MAX_RADIUS:
            raise ValueError(f'{name}: the target grid is {f[a]:.3g} times coarser than the source along source axis {"xyz"[a]}: the '
                             f'anti-aliasing filter would need a radius of {r[a]} voxels (at most {MAX_RADIUS})')
    return dict(factors=f, sigmas=s, radii=r, weights=[weights(v) for v in s])


def lowpass(dev_raw, code, shape, slope, inter, M, name='the volume'):
    """The low-pass the sampling matrix M asks for, on the device -> (fp32 [Z,Y,X] or None when no axis is filtered: nothing was
    launched, the non-finite voxels read as 0, the plan)."""
    from . import ops
    p = lowpass_plan(M, name)
    out, bad = ops.volume_lowpass(dev_raw, code, shape, slope, inter, p['weights'])
    return out, bad, p


# ---------------------------------------------------------------------------------------------------
# the pipeline's side
# ---------------------------------------------------------------------------------------------------
def add_flags(p):
    p.add_argument('--conform', action='store_true',
                   help='resample every input, the first included, once onto one axis-aligned grid of the training geometry (240 x 240 x 155 '
                        "voxels of 1 mm, stored LPS: BraTS), placed so that its centre lies on the centre of the first input's grid "
                        '(mudiff_hip.volume_conform): another voxel size or field of view reaches the generators at the scale they were '
                        'trained on and a tilted acquisition is de-obliqued.  Implies the resampling of --regrid for the inputs and for '
                        '--gt_volume / --eval_mask; everything is sampled, scored and written on that grid; conform_<t>.json next to the '
                        'prediction holds what was done')
    p.add_argument('--conform_shape', nargs=3, type=int, default=list(DEFAULT_SHAPE), metavar=('X', 'Y', 'Z'), help='the voxels of the conform grid')
    p.add_argument('--conform_spacing', nargs='+', type=float, default=list(DEFAULT_SPACING[:1]), metavar='MM',
                   help='the voxel size of the conform grid in mm: one value, or three (one per axis)')
    p.add_argument('--conform_to', type=str, default=DEFAULT_TARGET, metavar='CODE',
                   help='the orientation of the conform grid (as --reorient_to: the direction every storage axis runs towards)')
    p.add_argument('--conform_back', action='store_true',
                   help="with --conform: write predicted_<t>.nii.gz (and predicted_<t>_std.nii.gz) resampled onto the first input's own grid "
                        '(by --regrid_interp), with its affine and header (scored first, on the conform grid)')
    p.add_argument('--antialias', type=str, default=None, choices=['on', 'off'],
                   help='low-pass a volume on the GPU before a resampling that downsamples it (--conform, --regrid, --coregister; the '
                        '--gt_volume too, never the --eval_mask): a separable Gaussian per source axis whose FWHM, added in quadrature to '
                        'the source voxel, gives the target voxel, sigma = sqrt(f^2 - 1) / 2.355 source voxels for a sampling factor f > 1 '
                        '(an untuned default, not a measured optimum); an axis that is not downsampled is not filtered, and a resampling '
                        "that downsamples nothing is bit for bit what it is without the flag.  Default: 'on' under --conform, else 'off'")


def options_from(args):
    """A namespace's --conform flags and --antialias (any may be missing) -> IntakeOptions' `conform`: the keyword arguments of
    conform_grid, or None without --conform; and `antialias`: --antialias as a bool, on by default under --conform and off otherwise.
    ValueError, naming the flag, for a bad shape, spacing or code and for --conform_back on its own."""
    spacing = getattr(args, 'conform_spacing', None)
    grid = dict(shape=_shape3(getattr(args, 'conform_shape', None) or DEFAULT_SHAPE, '--conform_shape'),
                spacing=_spacing3(DEFAULT_SPACING if spacing is None else spacing), target=check_target(getattr(args, 'conform_to', DEFAULT_TARGET)))
    on = bool(getattr(args, 'conform', False))
    if getattr(args, 'conform_back', False) and not on:
        raise ValueError('--conform_back needs --conform')
    antialias = getattr(args, 'antialias', None)
    return dict(conform=grid if on else None, antialias=on if antialias is None else antialias in (True, 'on'))


def entry(raw, M, resampled, nonfinite=0, antialias=True):
    """What conform_<t>.json holds for one input: where it came from, what the sampling matrix M covers per source axis and what the
    anti-aliasing rule made of it (sigmas and radii all 0 with `antialias` off)."""
    from .volume_regrid import world_affine_of
    world = np.asarray(world_affine_of(raw.affine, raw.header), np.float64)
    f = factors(M)
    s = [sigma_of(v) if antialias else 0.0 for v in f]
    return {'shape_from': [int(v) for v in raw.shape], 'spacing_from': [float(np.sqrt((world[:3, v] ** 2).sum())) for v in range(3)],
            'obliquity_deg': obliquity_deg(world), 'factors': f, 'sigmas': s, 'radii': [radius(v) for v in s],
            'resampled': bool(resampled), 'nonfinite': int(nonfinite)}


def reference_of(ref, conform):
    """(shape, affine, header) of the conform grid of a first input whose own geometry is `ref` = (shape, affine, header); `conform`:
    IntakeOptions.conform.  The grid a prediction under --conform has, for the evaluation inputs to be checked and resampled against: the
    fp64 affine prepare_inputs resamples the inputs with, not its fp32 image in a header.  No voxel is moved."""
    from .volume_regrid import world_affine_of
    shape, affine = conform_grid(ref[0], world_affine_of(ref[1], ref[2]), **conform)
    return shape, affine, None                           # (no header: the fp64 affine itself is the grid, as in prepare_inputs)


def first_on_own_grid(first_raw, options):
    """What --conform_back resamples onto: the first input as stored, or under --reorient its geometry once reoriented
    (volume_reorient.reference_of: shape, affine, header; --reorient_back then takes it from there to the storage order)."""
    if options.reorient is None:
        return first_raw
    import types
    from .volume_reorient import reference_of as reoriented
    shape, affine, header = reoriented(first_raw, **options.reorient)[0]
    return types.SimpleNamespace(shape=tuple(shape), affine=affine, header=header)


def grid_name(shape, spacing):
    """'240x240x155@1mm'; an anisotropic spacing as '0.5x0.5x2mm'."""
    sp = _spacing3(spacing)
    mm = f'{sp[0]:g}' if sp[0] == sp[1] == sp[2] else 'x'.join(f'{v:g}' for v in sp)
    return 'x'.join(str(int(v)) for v in shape) + f'@{mm}mm'


def conform_suffix(entries, grid=None):
    """What a [done] line gains under --conform (nothing otherwise): ` | conform=240x240x155@1mm:T1,T2,FLAIR`, the names being the inputs
    that were resampled."""
    if not entries:
        return ''
    return f' | conform={grid}:' + ','.join(name for name, e in entries if e['resampled'])


def antialias_suffix(ran):
    """` | antialias=on` when a low-pass actually ran."""
    return ' | antialias=on' if ran else ''


def write_reports(entries, output_dir, target, grid=None):
    """conform_<t>.json next to the prediction: {'grid': name, 'inputs': {input name: entry}}.  -> its path."""
    return write_report_json('conform', {'grid': grid, 'inputs': {name: e for name, e in entries}}, output_dir, target)


def write_back(write, first_raw, grid_shape, grid_affine, device, interp='linear', antialias=True):
    """--conform_back: wraps a `write(path, vol, affine, header)` callable (volume.write_nifti, a cohort's deferred writer, or
    volume_reorient.write_back's wrapper) so that the volume it is given on the conform grid is resampled onto the first input's own grid
    (`first_raw`: shape, world affine, header; under --reorient the reoriented first input) with volume_regrid.regrid_to - `interp`, and
    the same anti-aliasing rule, which only acts where that grid is coarser - and written with the first input's affine and header."""
    from . import NIFTI_F4
    from .volume_intake import RawVolume
    from .volume_regrid import regrid_to, world_affine_of
    shape, world = first_raw.shape, world_affine_of(first_raw.affine, first_raw.header)
    grid_shape, grid_affine = _shape3(grid_shape), np.asarray(grid_affine, np.float64)

    def wrapped(path, vol, affine, header):
        data = np.ascontiguousarray(np.asarray(vol, np.float32).reshape(-1, order='F'))
        src = RawVolume(data, NIFTI_F4, '<', 1.0, 0.0, grid_shape, grid_affine, None)
        out = regrid_to(src, shape, world, device, mode=interp, antialias=antialias, name=os.path.basename(path))
        back = np.asarray(vol, np.float32) if out is src else out.values_float32()
        return write(path, back, first_raw.affine, first_raw.header)
    return wrapped
