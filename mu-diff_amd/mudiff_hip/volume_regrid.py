"""Inputs on different voxel grids (--regrid; csrc/volume_intake.hip: mud_volume_regrid).

The volume pipeline takes the geometry of its first input.  The reference (engine/test_volume.py:262-263) and this build refuse every
other input that does not have that shape, and mix inputs whose shapes agree but whose affines do not.  With --regrid each such volume
is resampled onto the first input's grid through the two affines before anything else sees it:

    stored voxels --upload--> mud_volume_regrid(inv(source affine) @ reference affine) --> fp32 [Z,Y,X] on the reference grid

trilinear for images (or, with --regrid_interp cubic, a cubic B-spline: mud_volume_bspline_coeffs + mud_volume_regrid_cubic, DESIGN.md
section 5.19), nearest neighbour for label volumes, zero outside the source's field of view.  The result is a volume like any
other (fp32, NIFTI_F4, the reference geometry): the host path downloads it and normalises it with numpy, the device path hands it to
the census / slab kernels where it is.  This is resampling between grids whose world coordinates already agree, not registration.

A volume's place in the world is NiftiHeader.world_affine: sform, else qform, else the pixdim diagonal (NIfTI-1's own order).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import NIFTI_F4, MudiffHipError, load, ptr, require_gpu
from .volume_intake import DEVICE_DTYPES, RawVolume, upload

MODES = {'linear': 0, 'nearest': 1}                     # the modes of mud_volume_regrid
MODES_HIGH = ('cubic',)                                  # the modes that run mud_volume_bspline_coeffs + mud_volume_regrid_cubic
INTERPS = ('linear',) + MODES_HIGH                       # --regrid_interp: how an image is resampled (a label volume: always nearest)


def add_flags(p):
    p.add_argument('--regrid', action='store_true',
                   help='accept inputs (and --gt_volume / --eval_mask) on other voxel grids: each volume that is not on the first '
                        "input's grid (shape and affine) is resampled onto it on the GPU through the affines before normalisation, "
                        'trilinearly (the label volume: nearest neighbour).  Resampling only: the volumes must already share one '
                        'world space (mudiff_hip.volume_regrid)')
    p.add_argument('--regrid_interp', type=str, default=INTERPS[0], choices=list(INTERPS),
                   help="how --regrid / --coregister resample an input (and --regrid the --gt_volume): 'linear' = trilinearly, which "
                        "softens the volume by an amount that depends on the sub-voxel offset; 'cubic' = with a cubic B-spline "
                        '(recursive prefilter + 4 x 4 x 4 gather on the GPU: mudiff_hip.volume_regrid), which keeps the sharpness of the '
                        'first input; zero background stays exactly zero.  The label volume stays nearest neighbour and the registration '
                        'search trilinear')


def options_from(args):
    """A namespace's --regrid / --regrid_interp (either may be missing) -> IntakeOptions' `regrid` and `interp`."""
    return dict(regrid=bool(getattr(args, 'regrid', False)), interp=str(getattr(args, 'regrid_interp', INTERPS[0])))


def regrid_suffix(names):
    """What a [done] line gains when --regrid resampled inputs (nothing otherwise: the lines as they were)."""
    names = list(names or ())
    return f" | regrid={','.join(names)}" if names else ''


def interp_suffix(interp, nonfinite=0):
    """What a [done] line gains under a non-default --regrid_interp (nothing by default: the lines as they were); `nonfinite`: the
    non-finite voxels the spline prefilter read as 0, named when there were any."""
    if interp == 'linear':
        return ''
    return f' | interp={interp}' + (f' nonfinite={int(nonfinite)}' if nonfinite else '')


def world_affine_of(affine, header):
    """The voxel -> world matrix of a read volume: the built-in reader's header knows qform (NiftiHeader.world_affine); nibabel's
    img.affine follows the same precedence already."""
    from .volume import NiftiHeader
    return header.world_affine if isinstance(header, NiftiHeader) else np.asarray(affine, np.float64)


def _affine44(a, what):
    a = np.asarray(a, np.float64)
    if a.shape != (4, 4) or not np.isfinite(a).all():
        raise ValueError(f'{what}: need a finite 4 x 4 affine, got {a.tolist() if a.size <= 16 else a.shape}')
    return a


def grid_matrix(src_affine, ref_affine):
    """inv(src) @ ref in fp64: reference voxel index -> source voxel coordinate.  ValueError for a singular or non-finite affine."""
    src, ref = _affine44(src_affine, 'source affine'), _affine44(ref_affine, 'reference affine')
    for a, what in ((src, 'source'), (ref, 'reference')):
        lin = a[:3, :3]
        scale = np.abs(lin).max()
        if scale == 0 or abs(np.linalg.det(lin / scale)) < 1e-12:      # (columns of a real grid are millimetres apart: far from this)
            raise ValueError(f'the {what} affine is singular')
    m = np.linalg.solve(src, ref)
    if not np.isfinite(m).all():
        raise ValueError('the source affine is singular')
    return m


def same_grid(shape_a, aff_a, shape_b, aff_b):
    """True iff the shapes are equal and the affines are equal once both are rounded to float32 (what a header stores: an exact
    comparison, no tolerance)."""
    if tuple(int(v) for v in shape_a) != tuple(int(v) for v in shape_b):
        return False
    a, b = np.asarray(aff_a, np.float64), np.asarray(aff_b, np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.astype(np.float32), b.astype(np.float32)))


def regrid(dev_raw, code, shape, slope, inter, M, out_shape, mode='linear', found=None, antialias=False, name=None):
    """mud_volume_regrid: the flat device array of a volume's stored voxels (datatype `code`, shape [SX,SY,SZ]) -> device fp32
    [Z,Y,X] on the grid of `out_shape` = (X,Y,Z).  M: grid_matrix(...) (4 x 4 or 3 x 4).  mode 'cubic': the value range
    (mud_volume_fg_range), the spline coefficients (mud_volume_bspline_coeffs: fp64, freed on return) and mud_volume_regrid_cubic; a dict
    `found` then receives `nonfinite`, the non-finite voxels that were read as 0.  `antialias` (--antialias; an
    image only, never mode 'nearest'): where M steps over more than one source voxel the volume first goes through the Gaussian low-pass
    volume_conform.lowpass_plan(M) asks for (mud_volume_lowpass) and its fp32 output is what is resampled; `found` then receives the plan
    as `antialias`, `lowpass` (True when a pass ran) and the non-finite voxels the filter read as 0 in `nonfinite`.  Where no axis needs
    filtering nothing is launched and the stored voxels are resampled as without it.  `name`: what an error calls the volume."""
    require_gpu(dev_raw)
    if mode not in MODES and mode not in MODES_HIGH:
        raise ValueError(f'mode must be one of {tuple(MODES) + MODES_HIGH}, got {mode!r}')
    if int(code) not in DEVICE_DTYPES:
        raise MudiffHipError(f'regrid: unsupported NIfTI datatype code {code}')
    SX, SY, SZ = (int(v) for v in shape)
    X, Y, Z = (int(v) for v in out_shape)
    if dev_raw.numel() != SX * SY * SZ or dev_raw.element_size() != np.dtype(DEVICE_DTYPES[int(code)]).itemsize or not dev_raw.is_contiguous():
        raise MudiffHipError(f'regrid: {dev_raw.numel()} voxels of {dev_raw.element_size()} bytes do not hold a {SX} x {SY} x {SZ} volume of '
                             f'datatype {code}')
    m = np.ascontiguousarray(np.asarray(M, np.float64)[:3, :4])
    if m.shape != (3, 4):
        raise ValueError(f'regrid: need a 3 x 4 or 4 x 4 matrix, got {np.shape(M)}')
    from . import ops
    bad = 0
    if antialias and mode != 'nearest':
        from . import volume_conform as VCF
        low, bad, plan = VCF.lowpass(dev_raw, int(code), (SX, SY, SZ), float(slope), float(inter), m, name or 'the volume')
        if found is not None:
            found.update(antialias={k: plan[k] for k in ('factors', 'sigmas', 'radii')}, lowpass=low is not None, nonfinite=bad)
        if low is not None:
            dev_raw, code, slope, inter = low.reshape(-1), NIFTI_F4, 1.0, 0.0
    out = torch.empty(max(Z, 0), max(Y, 0), max(X, 0), device=dev_raw.device, dtype=torch.float32)
    if mode in MODES_HIGH:
        from .volume_foreground import unkey
        rng = ops.volume_fg_range(dev_raw, int(code), (SX, SY, SZ), float(slope), float(inter)).cpu().numpy().view(np.uint32)
        lo, hi = (unkey(~int(rng[0])), unkey(rng[1])) if int(rng[2]) else (0.0, 0.0)      # the finite values that are != 0 ...
        lo, hi = min(lo, 0.0), max(hi, 0.0)                                               # ... widened to contain 0
        coeffs = torch.empty(SZ, SY, SX, device=dev_raw.device, dtype=torch.float64)
        seen = torch.empty(1, device=dev_raw.device, dtype=torch.int32)
        ops._launch('volume_bspline_coeffs', dev_raw.device, load().mud_volume_bspline_coeffs, ptr(dev_raw), int(code), SX, SY, SZ, float(slope),
                    float(inter), ptr(coeffs), ptr(seen), ops.STREAM, nbytes=float(dev_raw.numel() * (3 * dev_raw.element_size() + 80)))
        ops._launch('volume_regrid_cubic', dev_raw.device, load().mud_volume_regrid_cubic, ptr(coeffs), SX, SY, SZ, ptr(dev_raw), int(code),
                    float(slope), float(inter), (C.c_double * 12)(*m.reshape(-1).tolist()), lo, hi, X, Y, Z, ptr(out), ops.STREAM,
                    nbytes=float(8 * coeffs.numel() + dev_raw.numel() * dev_raw.element_size() + 4 * out.numel()))
        if found is not None:
            found['nonfinite'] = bad + int(seen.cpu().numpy().view(np.uint32)[0])
        del coeffs                                            # (stream-ordered: the allocator reuses it after the launch above)
        return out
    ops._launch('volume_regrid', dev_raw.device, load().mud_volume_regrid, ptr(dev_raw), int(code), SX, SY, SZ, float(slope), float(inter),
                (C.c_double * 12)(*m.reshape(-1).tolist()), MODES[mode], X, Y, Z, ptr(out), ops.STREAM,
                nbytes=float(dev_raw.numel() * dev_raw.element_size() + 4 * out.numel()))
    return out


class RegriddedVolume(RawVolume):
    """A RawVolume whose voxels live on the device (`dev`: fp32 [Z,Y,X], the reference geometry).  volume_intake.upload hands `dev`
    on as it is; `data` (the flat fp32 host array in file order) is downloaded on first use and kept."""

    def __init__(self, dev, shape, affine, header):
        self._host = None
        super().__init__(None, NIFTI_F4, '<', 1.0, 0.0, shape, affine, header)
        self.dev = dev

    @property
    def data(self):
        if self._host is None:
            self._host = self.dev.reshape(-1).cpu().numpy()
        return self._host

    @data.setter
    def data(self, value):
        self._host = value

    def values_float32(self):
        """The volume as an F-ordered fp32 [X,Y,Z] host array (a view of `data`)."""
        return self.data.reshape(self.shape, order='F')


def regrid_to(raw, ref_shape, ref_affine, device, mode='linear', header=None, world=None, found=None, antialias=False, name=None):
    """A RawVolume -> the same volume on the grid (ref_shape, ref_affine): a RegriddedVolume (fp32, NIFTI_F4, slope 1, inter 0, that
    geometry; `header`: the reference's) ready for volume_intake.condition_from_raw.  A volume already on that grid is returned
    untouched.  The source's place in the world is world_affine_of(raw.affine, raw.header).  `world` (--coregister,
    mudiff_hip.volume_coreg): a 4 x 4 matrix W that takes a world point of the reference to the source's world, so that the sampling
    matrix is inv(source affine) @ W @ reference affine; with a W that is not the identity the volume is resampled even on its own grid.
    `mode`: 'linear', 'cubic' (an image) or 'nearest' (a label volume); `found`, `antialias`, `name`: see regrid."""
    if len(raw.shape) != 3 or len(ref_shape) != 3:
        raise ValueError(f'regrid: expected 3D volumes, got shapes {tuple(raw.shape)} and {tuple(ref_shape)}')
    src_affine = world_affine_of(raw.affine, raw.header)
    moved = world is not None and not np.array_equal(np.asarray(world, np.float64), np.eye(4))
    if not moved and same_grid(raw.shape, src_affine, ref_shape, ref_affine):
        return raw
    M = grid_matrix(src_affine, _affine44(world, 'world transform') @ _affine44(ref_affine, 'reference affine') if moved else ref_affine)
    if antialias:
        dev = regrid(upload(raw, device), raw.code, raw.shape, *raw.scaling, M, ref_shape, mode, found, antialias=True, name=name)
    else:
        dev = regrid(upload(raw, device), raw.code, raw.shape, *raw.scaling, M, ref_shape, mode, found)
    return RegriddedVolume(dev, ref_shape, np.asarray(ref_affine, np.float64), header)


def eval_onto_grid(ref_shape, ref_affine, gt_raw, mask_raw, device, names=('gt_volume', 'eval_mask'), interp='linear', found=None,
                   antialias=False):
    """The evaluation inputs on the reference grid: the ground truth by `interp` (--regrid_interp: trilinearly by default), the label
    volume by nearest neighbour, always.  A dict `found` has the non-finite voxels a cubic resampling read as 0 added to its `nonfinite`.
    `antialias`: the ground truth goes through regrid's low-pass first (the label volume never); `found` gets `lowpass` when one ran.
    -> (gt [X,Y,Z] float64 as volume.read_nifti returns it, label or None, the names of what was resampled)."""
    out, done = [], []
    for raw, mode, name in ((gt_raw, interp, names[0]), (mask_raw, 'nearest', names[1])):
        if raw is None:
            out.append(None)
            continue
        if mode not in INTERPS and mode != 'nearest':
            raise ValueError(f'interp must be one of {INTERPS}, got {mode!r}')
        seen = {}
        more = dict(antialias=True, name=name) if antialias and mode != 'nearest' else {}
        r = regrid_to(raw, ref_shape, ref_affine, device, mode, found=seen, **more)
        if found is not None:
            found['nonfinite'] = found.get('nonfinite', 0) + seen.get('nonfinite', 0)
            if seen.get('lowpass'):
                found['lowpass'] = True
        if r is not raw:
            done.append(name)
            out.append(r.values_float32().astype(np.float64))
        else:
            out.append(raw.values_float64())
    return out[0], out[1], done
