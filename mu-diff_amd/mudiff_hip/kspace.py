"""Sample a target that was acquired undersampled in k-space (--known_kspace; csrc/kspace.hip: mud_fft2_c2c, mud_kspace_constrain;
DESIGN.md section 5.26).

--known_volume keeps the voxels of the target that were acquired.  An accelerated acquisition is partly there in another way: every
slice is present, but only some phase-encode lines of its k-space are, or only the low-resolution centre of a fast scout.  With
--known_kspace PATTERN the slices of --known_volume K are measured retrospectively, in the established protocol of guided
reconstruction (a magnitude image, fastMRI-style Cartesian masks), and the sampler keeps the measured coefficients:

    K --known_region's road--> the prediction's grid --norm, resize--> k [n,S,S] --ops.fft2--> y = M_eff * F(k) --> sampler (every step)

F is the unitary 2D DFT on the sampler's S x S grid (S = --image_size, a power of two in [16, 512]; DC at [0,0]).  M is one 0/1 mask
per volume, numpy, a function of the flags and --seed alone.  k is real, so F(k) is Hermitian and a measured coefficient gives its
mirror: the sampler works with M_eff[u,v] = M[u,v] | M[-u mod S, -v mod S], and the report holds both sampling fractions.  After the
reverse step executed with t = i the measured coefficients of x are replaced by those of q_sample(k, i), after the last by y itself
(GraphSampler.sample_keyed's `kspace`, kind ops.KIND_KSPACE; the draw and --known_resample: mudiff_hip.constraints, section 5.24a).

A slice is measured when K is finite and fully covered on it after resampling (known_region's coverage) and --known_drop_slices does
not name it: `this slice was not measured` is a zero mask row, and the slice is sampled freely.  --known_mask is refused: a voxel mask
has no meaning in k-space.

There is no final paste.  Consistency holds on the sampler's grid: kspace_<t>.json lists, per slice, |M_eff * (F(x) - y)| / |y| of the
sampler's result before it is mapped to [0,1].  It survives the affine [0,1] map (away from the clip) and an ensemble's mean; it does
not survive clipping, --resize_back, the median or the quantile maps.

This is the single-coil, real-image, retrospective model of the research on guided accelerated acquisition.  A multi-coil
acquisition is --known_sense (mudiff_hip.sense, section 5.32); complex raw data is out of scope.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .constraints import Constraint, KSpaceRows, need_keyed_seed, need_known_volume, relative_residual

PATTERNS = ('equispaced', 'random', 'lowres', 'file')
DEFAULT_ACCEL, DEFAULT_CENTER, DEFAULT_AXIS = 4, 0.08, 0


def add_flags(p):
    p = p.later() if hasattr(p, 'later') else p          # volume.VolumeParser: the lists of the parsers before this one are pinned
    p.add_argument('--known_kspace', type=str, default=None, choices=list(PATTERNS),
                   help='with --known_volume K: K was acquired undersampled in k-space.  Its slices are measured retrospectively with this '
                        'sampling pattern and the measured coefficients are re-imposed after every reverse step (mudiff_hip.kspace, DESIGN.md '
                        'section 5.26); --known_drop_slices then means `this slice was not measured`')
    p.add_argument('--kspace_accel', type=int, default=None, metavar='R',
                   help=f'with --known_kspace equispaced / random: the acceleration, an integer >= 1 (default {DEFAULT_ACCEL})')
    p.add_argument('--kspace_center', type=float, default=None, metavar='F',
                   help=f'the fraction of fully sampled central lines (fastMRI\'s convention); for lowres the kept block is the central '
                        f'round(F * S)^2 square (default {DEFAULT_CENTER})')
    p.add_argument('--kspace_axis', type=int, default=None, choices=[0, 1], help=f'the phase-encode axis of the slice (default {DEFAULT_AXIS})')
    p.add_argument('--kspace_mask_file', type=str, default=None, metavar='M.npy',
                   help='with --known_kspace file: uint8 [S, S], non-zero = measured, centred (DC at [S/2, S/2])')
    p.add_argument('--kspace_zero_filled', action='store_true',
                   help='also write zero_filled_<t>.nii.gz = Re F^H y, the reconstruction without the model (scored too under --gt_volume)')


def pattern_options(flag, prefix, pattern, accel, center, axis, mask_file, axis_checked=True):
    """The sampling pattern of --known_kspace or --known_multislice (`flag`; its dependents are `prefix`accel, ...) as given (None: the
    default) -> dict(accel, center, axis, mask_file).  ValueError naming the flag for a bad value.  --known_kspace has never refused an
    axis (`axis_checked` False): build_mask takes every axis but 0 as 1."""
    accel = DEFAULT_ACCEL if accel is None else accel
    center = DEFAULT_CENTER if center is None else float(center)
    axis = DEFAULT_AXIS if axis is None else axis
    if int(accel) != accel or accel < 1:
        raise ValueError(f'{prefix}accel must be an integer >= 1, got {accel}')
    if not 0.0 <= center <= 1.0:
        raise ValueError(f'{prefix}center must lie in [0, 1], got {center}')
    if axis_checked and axis not in (0, 1):
        raise ValueError(f'{prefix}axis must be 0 or 1, got {axis}')
    if (pattern == 'file') != (mask_file is not None):
        raise ValueError(f'{prefix}mask_file goes with {flag} file, and that pattern needs it')
    return dict(accel=int(accel), center=center, axis=int(axis), mask_file=mask_file)


def options_from(args):
    """A namespace's --known_kspace / --kspace_* flags (any may be missing) -> None without --known_kspace, else dict(pattern, accel,
    center, axis, mask_file, zero_filled).  ValueError, naming the flag, for a dependent flag without --known_kspace, --known_kspace
    without --known_volume (a cohort's namespace excepted: its K is the manifest's `known` column) or with --known_mask, an --image_size
    the transform does not take, and a bad value."""
    pattern = getattr(args, 'known_kspace', None)
    accel, center, axis = (getattr(args, f, None) for f in ('kspace_accel', 'kspace_center', 'kspace_axis'))
    mask_file, zero_filled = getattr(args, 'kspace_mask_file', None), bool(getattr(args, 'kspace_zero_filled', False))
    if pattern is None:
        for flag, given in (('--kspace_accel', accel is not None), ('--kspace_center', center is not None), ('--kspace_axis', axis is not None),
                            ('--kspace_mask_file', mask_file is not None), ('--kspace_zero_filled', zero_filled)):
            if given:
                raise ValueError(f'{flag} needs --known_kspace')
        return None
    if pattern not in PATTERNS:
        raise ValueError(f'--known_kspace must be one of {PATTERNS}, got {pattern!r}')
    need_known_volume(args, '--known_kspace')
    if getattr(args, 'known_mask', None) is not None:
        raise ValueError('--known_kspace cannot be combined with --known_mask (a voxel mask has no meaning in k-space; '
                         'use --known_drop_slices for slices that were not measured)')
    from .ops import kspace_size_ok
    size = getattr(args, 'image_size', None)
    if size is not None and not kspace_size_ok(size):
        raise ValueError(f'--known_kspace needs an --image_size that is a power of two in [16, 512], got {size}')
    sampling = pattern_options('--known_kspace', '--kspace_', pattern, accel, center, axis, mask_file, axis_checked=False)
    need_keyed_seed(args, '--known_kspace')
    return dict(pattern=pattern, **sampling, zero_filled=zero_filled)


# ---------------------------------------------------------------------------------------------------
# sampling masks: numpy, uint8 [S, S] in the kernel's order (DC at [0, 0]), deterministic in the seed
# ---------------------------------------------------------------------------------------------------
def center_lines(S, fraction):
    """bool [S], centred: the round(S * fraction) fully sampled central lines, placed as fastMRI places them."""
    n = int(round(S * float(fraction)))
    lines = np.zeros(S, bool)
    pad = (S - n + 1) // 2
    lines[pad:pad + n] = True
    return lines


def line_pattern(S, pattern, accel, center, seed):
    """bool [S], centred (DC at S // 2): the measured phase-encode lines.  equispaced: every accel-th line from an offset drawn from the
    seed, and the central lines; random: each other line with the probability that makes S / accel lines in expectation (fastMRI's
    RandomMaskFunc), and the central lines."""
    lines = center_lines(S, center)
    rng = np.random.default_rng([int(seed) & 0xFFFFFFFFFFFFFFFF, 0x6B73])
    if pattern == 'equispaced':
        lines[int(rng.integers(0, accel))::accel] = True
    elif pattern == 'random':
        n_low = int(lines.sum())
        prob = min(1.0, max(0.0, (S / accel - n_low) / max(S - n_low, 1)))
        lines |= rng.uniform(size=S) < prob
    else:
        raise ValueError(f'line_pattern: equispaced or random, got {pattern!r}')
    return lines


def build_mask(S, pattern, accel=DEFAULT_ACCEL, center=DEFAULT_CENTER, axis=DEFAULT_AXIS, seed=0, mask_file=None):
    """The sampling mask M of one volume: uint8 [S, S], DC at [0, 0].  `axis`: the phase-encode axis (lines of the other axis are
    measured whole).  lowres: the central round(center * S)^2 square.  file: `mask_file` (.npy, uint8 [S, S], centred) or an array."""
    S = int(S)
    if pattern == 'file':
        m = np.load(mask_file) if isinstance(mask_file, (str, os.PathLike)) else np.asarray(mask_file)
        if m.shape != (S, S):
            raise ValueError(f'--kspace_mask_file: expected a [{S}, {S}] array (the sampler\'s grid), got {m.shape}')
        centred = m != 0
    elif pattern == 'lowres':
        c = center_lines(S, center)
        centred = c[:, None] & c[None, :]
    else:
        lines = line_pattern(S, pattern, int(accel), center, seed)
        centred = np.broadcast_to(lines[:, None] if int(axis) == 0 else lines[None, :], (S, S))
    return np.ascontiguousarray(np.fft.ifftshift(centred)).astype(np.uint8)


def symmetrise(mask):
    """M_eff[u, v] = M[u, v] | M[-u mod S, -v mod S]: a real image's measured coefficient gives its mirror."""
    m = np.asarray(mask) != 0
    return (m | np.roll(m[::-1, ::-1], (1, 1), (0, 1))).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------
# the measurement of one prediction
# ---------------------------------------------------------------------------------------------------
class KSpaceMeasurement(Constraint):
    """What the samplers take for one prediction: `y` complex64 [n,S,S] = M_eff * F(k) and `mask` uint8 [n,S,S] (M_eff on a measured
    slice, zeros on one that is not) on the device, n the slab's slices; `report`: kspace_<t>.json; `resample`: --known_resample.
    `record` collects the data-consistency residual of what the sampler returned."""

    def __init__(self, y, mask, report, resample, options):
        self.y, self.mask, self.report, self.resample, self.options = y, mask, report, int(resample), options
        self.n = int(y.shape[0])
        self.y_norm = torch.linalg.vector_norm(y.flatten(1), dim=1)
        self.residual = torch.zeros(y.shape[0], device=y.device, dtype=torch.float32)
        self.x_norm = torch.zeros_like(self.residual)

    tag = 'kspace'
    done_suffix = lambda self: suffix(self)      # noqa: E731
    baseline = lambda self: ('zero_filled', self.zero_filled()) if self.options['zero_filled'] else None      # noqa: E731

    def for_rows(self, slices, samples, m):
        """A padded row (from m on) repeats the last item's coefficients and mask; only the first m rows are recorded."""
        idx = torch.as_tensor(slices, dtype=torch.int64, device=self.y.device)
        return KSpaceRows(self.y.index_select(0, idx), self.mask.index_select(0, idx), idx[:m])

    def record(self, bound, x, x_new=None):
        """x [B,1,S,S]: what the sampler returned (in [-1,1], before any map) for the batch that for_rows bound: keeps, per slice, the
        largest |M_eff * (F(x) - y)| / |y| seen over its real rows (an ensemble records every sample)."""
        from . import ops
        idx = bound.idx
        x = x[:idx.shape[0]]
        F = ops.fft2(x[:, 0].contiguous())
        d = torch.where(self.mask.index_select(0, idx) != 0, F - self.y.index_select(0, idx), torch.zeros((), device=F.device, dtype=F.dtype))
        self.residual.scatter_reduce_(0, idx, relative_residual(d.flatten(1), self.y_norm.index_select(0, idx)), 'amax')
        self.x_norm.scatter_reduce_(0, idx, torch.linalg.vector_norm(x.flatten(1), dim=1), 'amax')

    def zero_filled(self):
        """Re F^H y [n,S,S] in [-1,1] terms: the reconstruction without the model."""
        from . import ops
        return ops.fft2(self.y, inverse=True).real.contiguous()

    def finish(self):
        """The report with the residuals put in (None for a slice that was not measured)."""
        res = self.residual.cpu().tolist()
        self.report['residual_per_slice'] = [r if m else None for r, m in zip(res, self.report['measured_per_slice'])]
        self.report['max_residual'] = max([r for r, m in zip(res, self.report['measured_per_slice']) if m], default=None)
        self.report['y_norm_per_slice'] = self.y_norm.cpu().tolist()       # |y| and the largest |x|: what the residual's rounding scales with
        self.report['x_norm_per_slice'] = self.x_norm.cpu().tolist()
        return self.report


def measure(region, s0, s1, size, options, seed, device):
    """known_region.KnownRegion (K on the prediction's grid: --norm applied, its known mask = coverage AND finite AND not dropped AND
    slab) -> KSpaceMeasurement for the slab s0..s1 on the S x S sampler grid."""
    from . import known_region as KR
    from . import ops
    S = int(size)
    k, vmask = KR.sampler_inputs(region, s0, s1, S, device)                      # [n,1,S,S] each, resized like the conditions
    measured = vmask.flatten(1).min(1).values != 0                               # every pixel of the slice known
    M = build_mask(S, options['pattern'], options['accel'], options['center'], options['axis'], seed, options['mask_file'])
    M_eff = symmetrise(M)
    mask = (torch.from_numpy(M_eff).to(device)[None] * measured.to(torch.uint8)[:, None, None]).contiguous()
    F = ops.fft2(k[:, 0].contiguous())
    y = torch.where(mask != 0, F, torch.zeros((), device=device, dtype=F.dtype)).contiguous()
    flags = [bool(v) for v in measured.cpu().tolist()]
    report = dict(pattern=options['pattern'], accel=options['accel'], center=options['center'], axis=options['axis'],
                  mask_file=options['mask_file'], image_size=S, slab=[int(s0), int(s1)], given_fraction=float(M.mean()),
                  effective_fraction=float(M_eff.mean()), measured_slices=sum(flags), unmeasured_slices=len(flags) - sum(flags),
                  measured_per_slice=flags, drop_slices=region.report['drop_slices'], resample=region.resample,
                  resampled=region.report['resampled'])
    return KSpaceMeasurement(y, mask, report, region.resample, options)


def suffix(measurement):
    """What a [done] line gains (nothing without --known_kspace)."""
    if measurement is None:
        return ''
    r = measurement.report
    return f" | kspace={r['pattern']} x{r['accel']} ({r['effective_fraction']:.3f})"

