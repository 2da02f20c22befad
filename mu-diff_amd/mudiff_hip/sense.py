"""Sample a target that was acquired accelerated on several coils (--known_sense; csrc/sense.hip: mud_sense_measure, mud_sense_adjoint,
mud_sense_constrain).

--known_kspace measures the slices of --known_volume K on one coil: y = M F(k), and the projection onto the measurement is closed form.
Real accelerated scans are multi-coil.  With --known_sense PATTERN every slice is measured through Nc coil sensitivities,

    K --known_region's road--> the prediction's grid --norm, resize--> k [n,S,S] --ops.sense_measure--> y_c = M F(C_c k) (+ noise)
      --ops.sense_adjoint--> A^H y [n,S,S] --> sampler (every step)

F is the unitary 2D DFT of mudiff_hip.kspace, M kspace.build_mask's pattern, NOT symmetrised (C_c k is complex: a coefficient does not
give its mirror), C the sensitivities: --sense_maps M.npy (complex64 [Nc,S,S], unit root-sum-of-squares wherever not all zero) or the
smooth synthetic ones of coil_maps (--sense_coils N; not a coil simulation).  With --sense_noise sigma the measured coefficients carry
sigma (n_re + i n_im), keyed normals of kind ops.KIND_SENSE_MEAS under (--seed, step 0) with the key (global slice, coil) and rows of
2 S^2 (element 2 j: the real part of coefficient j, 2 j + 1: its imaginary part), so y depends neither on the batch size nor on the slab.

N = A^H A mixes coils and aliases, and with enough coils the measurement determines the image alone, so the step after the reverse step
executed with t = i is a regularised one: x = argmin |x - x_new|^2 + lambda |A (x - s eta) - a y|^2 with a, s of level i (clean at
i = 0) and eta a keyed normal of kind ops.KIND_SENSE (the draw and --known_resample: mudiff_hip.constraints, section 5.24a), solved by
--sense_iters conjugate-gradient iterations on the device (constraints.SenseRows).  The defaults of --sense_lambda and --sense_iters
are untuned.

A slice is measured under mudiff_hip.kspace's rule (K finite and fully covered, not named by --known_drop_slices); any other slice
gets a zero mask row and is sampled freely.  There is no final paste.  sense_<t>.json lists, per slice and over the real rows of an
ensemble, the residual |M F(C x) - y| / |y| of the sampler's result before the [0,1] map, the same for the last step's x_new, and the
largest |r| / |b| the conjugate gradients ended with.  --sense_baseline also writes and scores sense_baseline_<t>.nii.gz =
lambda (I + lambda N)^-1 A^H y, the regularised SENSE reconstruction without the model: the same kernel applied clean to x_new = 0.

Out of scope: estimating sensitivities from calibration lines, raw multi-coil k-space files, complex-valued targets, non-Cartesian
patterns, per-slice masks from a file, a data-dependent stopping rule, the uncaptured sampler path and the PNG driver.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from .constraints import Constraint, SenseRows, need_keyed_seed, need_known_volume
from .kspace import PATTERNS, build_mask, pattern_options

DEFAULT_COILS, DEFAULT_LAMBDA, DEFAULT_ITERS = 8, 8.0, 12      # (lambda and iters: untuned)
MAX_COILS, MAX_ITERS, MAPS_TOLERANCE = 32, 64, 1e-3
_OTHERS = ('known_kspace', 'known_thick', 'known_multislice', 'known_thick_volume', 'known_lowres_volume')
_CHUNK = 1 << 28                      # coefficients per measurement launch (the kernels take < 2^31)


def add_flags(p):
    p = p.later() if hasattr(p, 'later') else p          # volume.VolumeParser: the lists of the parsers before this one are pinned
    p.add_argument('--known_sense', type=str, default=None, choices=list(PATTERNS),
                   help='with --known_volume K: K was acquired accelerated on several coils.  Its slices are measured retrospectively through '
                        'the coil sensitivities with this sampling pattern, and after every reverse step the result is pulled towards the '
                        'measurement by a regularised conjugate-gradient step (mudiff_hip.sense, DESIGN.md section 5.32); '
                        '--known_drop_slices then means `this slice was not measured`')
    p.add_argument('--sense_accel', type=int, default=None, metavar='R', help='with --known_sense equispaced / random: the acceleration (default 4)')
    p.add_argument('--sense_center', type=float, default=None, metavar='F', help='the fraction of fully sampled central lines (default 0.08)')
    p.add_argument('--sense_axis', type=int, default=None, help='the phase-encode axis of the slice, 0 or 1 (default 0)')
    p.add_argument('--sense_mask_file', type=str, default=None, metavar='M.npy',
                   help='with --known_sense file: uint8 [S, S], non-zero = measured, centred (DC at [S/2, S/2])')
    p.add_argument('--sense_coils', type=int, default=None, metavar='N',
                   help=f'the number of smooth synthetic coil sensitivities, 1..{MAX_COILS} (default {DEFAULT_COILS}); not with --sense_maps')
    p.add_argument('--sense_maps', type=str, default=None, metavar='M.npy',
                   help=f'coil sensitivities, complex64 [Nc, S, S] with Nc <= {MAX_COILS} and sum_c |C_c|^2 = 1 wherever they are not all zero')
    p.add_argument('--sense_lambda', type=float, default=None, metavar='L',
                   help=f'the weight of the data term, finite and >= 0 (default {DEFAULT_LAMBDA:g}, untuned)')
    p.add_argument('--sense_iters', type=int, default=None, metavar='K',
                   help=f'conjugate-gradient iterations per step, 1..{MAX_ITERS} (default {DEFAULT_ITERS}, untuned)')
    p.add_argument('--sense_noise', type=float, default=None, metavar='SIGMA',
                   help='the standard deviation of the measurement noise per real component, in the units of the [-1,1] image (default 0)')
    p.add_argument('--sense_baseline', action='store_true',
                   help='also write sense_baseline_<t>.nii.gz = lambda (I + lambda N)^-1 A^H y, the regularised SENSE reconstruction without '
                        'the model (scored too under --gt_volume)')


def options_from(args):
    """A namespace's --known_sense / --sense_* flags (any may be missing) -> None without --known_sense, else dict(pattern, accel, center,
    axis, mask_file, coils, maps, lam, iters, noise, baseline).  ValueError, naming the flag, for a dependent flag without --known_sense,
    --known_sense without --known_volume (a cohort's namespace excepted), with --known_mask or with any other --known_* mode, an
    --image_size the transform does not take, a bad value and a bad --seed."""
    pattern = getattr(args, 'known_sense', None)
    given = {f: getattr(args, f, None) for f in ('sense_accel', 'sense_center', 'sense_axis', 'sense_mask_file', 'sense_coils', 'sense_maps',
                                                 'sense_lambda', 'sense_iters', 'sense_noise')}
    baseline = bool(getattr(args, 'sense_baseline', False))
    if pattern is None:
        for f, v in list(given.items()) + [('sense_baseline', baseline or None)]:
            if v is not None:
                raise ValueError(f'--{f} needs --known_sense')
        return None
    if pattern not in PATTERNS:
        raise ValueError(f'--known_sense must be one of {PATTERNS}, got {pattern!r}')
    need_known_volume(args, '--known_sense')
    if getattr(args, 'known_mask', None) is not None:
        raise ValueError('--known_sense cannot be combined with --known_mask (a voxel mask has no meaning in k-space; '
                         'use --known_drop_slices for slices that were not measured)')
    for other in _OTHERS:
        if getattr(args, other, None) is not None:
            raise ValueError(f'--known_sense cannot be combined with --{other}: one measurement model per run')
    from .ops import kspace_size_ok
    size = getattr(args, 'image_size', None)
    if size is not None and not kspace_size_ok(size):
        raise ValueError(f'--known_sense needs an --image_size that is a power of two in [16, 512], got {size}')
    sampling = pattern_options('--known_sense', '--sense_', pattern, given['sense_accel'], given['sense_center'], given['sense_axis'],
                               given['sense_mask_file'])
    coils, maps = given['sense_coils'], given['sense_maps']
    if coils is not None and maps is not None:
        raise ValueError('--sense_coils cannot be combined with --sense_maps: the file says how many coils there are')
    coils = DEFAULT_COILS if coils is None else coils
    if int(coils) != coils or not 1 <= coils <= MAX_COILS:
        raise ValueError(f'--sense_coils must be an integer in [1, {MAX_COILS}], got {coils}')
    lam = DEFAULT_LAMBDA if given['sense_lambda'] is None else float(given['sense_lambda'])
    if not (lam >= 0.0 and math.isfinite(lam)):
        raise ValueError(f'--sense_lambda must be finite and >= 0, got {lam}')
    iters = DEFAULT_ITERS if given['sense_iters'] is None else given['sense_iters']
    if int(iters) != iters or not 1 <= iters <= MAX_ITERS:
        raise ValueError(f'--sense_iters must be an integer in [1, {MAX_ITERS}], got {iters}')
    noise = 0.0 if given['sense_noise'] is None else float(given['sense_noise'])
    if not (noise >= 0.0 and math.isfinite(noise)):
        raise ValueError(f'--sense_noise must be finite and >= 0, got {noise}')
    need_keyed_seed(args, '--known_sense')
    return dict(pattern=pattern, **sampling, coils=int(coils), maps=maps, lam=lam, iters=int(iters), noise=noise, baseline=baseline)


# ---------------------------------------------------------------------------------------------------
# coil sensitivities: numpy, complex64 [Nc, S, S]
# ---------------------------------------------------------------------------------------------------
def coil_maps(S, Nc):
    """The default maps: Nc smooth synthetic sensitivities on the S x S grid, Gaussian magnitudes centred on a ring of radius 0.75 around
    the image with a linear phase each, normalised to unit root-sum-of-squares; fp64, rounded once to complex64.  Not a coil simulation."""
    S, Nc = int(S), int(Nc)
    g = (np.arange(S) - S // 2) / S
    u, v = np.meshgrid(g, g, indexing='ij')
    theta = 2 * np.pi * (np.arange(Nc) + 0.5) / Nc
    ct, st = np.cos(theta)[:, None, None], np.sin(theta)[:, None, None]
    m = np.exp(-((u - 0.75 * ct) ** 2 + (v - 0.75 * st) ** 2) / (2 * 0.6 ** 2))
    phi = theta[:, None, None] + np.pi * (u * ct + v * st)
    return (m * np.exp(1j * phi) / np.sqrt((m ** 2).sum(0))).astype(np.complex64)


def load_maps(path, S):
    """--sense_maps: a .npy file (or an array) -> complex64 [Nc, S, S].  ValueError naming the flag for another shape or type, more than
    MAX_COILS coils, a value that is not finite, and a root-sum-of-squares that leaves 1 by more than MAPS_TOLERANCE where the maps are
    not all zero."""
    c = np.load(path) if isinstance(path, (str, os.PathLike)) else np.asarray(path)
    if c.ndim != 3 or c.shape[1:] != (int(S), int(S)) or not 1 <= c.shape[0] <= MAX_COILS or not np.iscomplexobj(c):
        raise ValueError(f'--sense_maps: expected a complex [Nc, {S}, {S}] array (the sampler\'s grid) with 1 <= Nc <= {MAX_COILS}, got '
                         f'{c.dtype} {c.shape}')
    c = np.ascontiguousarray(c, dtype=np.complex64)
    if not np.isfinite(c.view(np.float32)).all():
        raise ValueError('--sense_maps: a value is not finite')
    rss = (np.abs(c.astype(np.complex128)) ** 2).sum(0)
    off = np.abs(rss - 1.0)[rss > 0]
    if off.size and float(off.max()) > MAPS_TOLERANCE:
        raise ValueError(f'--sense_maps: sum_c |C_c|^2 must be 1 wherever the maps are not all zero (within {MAPS_TOLERANCE:g}), it leaves 1 by '
                         f'{float(off.max()):.3g}')
    return c


# ---------------------------------------------------------------------------------------------------
# the measurement of one prediction
# ---------------------------------------------------------------------------------------------------
def _chunks(n, per_slice):
    step = max(1, _CHUNK // per_slice)
    return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


def _norms(v):
    """|v| per row of [rows, ...] (real or complex), summed in fp64 and rounded once to fp32: a row's value does not depend on how many
    rows the batch holds (an fp32 reduction's order does)."""
    v = torch.view_as_real(v) if v.is_complex() else v
    return v.flatten(1).double().square().sum(1).sqrt().float()


class SenseMeasurement(Constraint):
    """What the samplers take for one prediction: `ahy` fp32 [n,S,S] = A^H y, `mask` uint8 [n,S,S] (M on a measured slice, zeros on one
    that is not) and `maps` complex64 [Nc,S,S] on the device, n the slab's slices; `y` complex64 [n,Nc,S,S], kept for the report alone;
    `report`: sense_<t>.json; `resample`: --known_resample.  `record` collects the residuals of what the sampler returned."""

    tag = 'sense'

    def __init__(self, y, ahy, mask, maps, report, resample, options):
        self.y, self.ahy, self.mask, self.maps, self.report, self.resample, self.options = y, ahy, mask, maps, report, int(resample), options
        self.n = int(y.shape[0])
        self.y_norm = _norms(y)
        self.residual = torch.zeros(self.n, device=y.device, dtype=torch.float32)
        self.residual_before, self.cg_residual, self.x_norm = (torch.zeros_like(self.residual) for _ in range(3))

    def done_suffix(self):
        return suffix(self)

    def baseline(self):
        return ('sense_baseline', self.reconstruction()) if self.options['baseline'] else None

    def for_rows(self, slices, samples, m):
        """A padded row (from m on) repeats the last item's measurement; only the first m rows are recorded."""
        idx = torch.as_tensor(slices, dtype=torch.int64, device=self.y.device)
        return SenseRows(self.ahy.index_select(0, idx), self.mask.index_select(0, idx), self.maps, self.options['lam'], self.options['iters'], idx[:m])

    def _residual(self, x, idx):
        from . import ops
        d = ops.sense_measure(x[:, 0].contiguous(), self.maps, self.mask.index_select(0, idx)) - self.y.index_select(0, idx)
        r, den = _norms(d), self.y_norm.index_select(0, idx)
        return torch.where(den > 0, r / den.clamp_min(1e-30), torch.zeros_like(r))      # (constraints.relative_residual's rule)

    def record(self, bound, x, x_new=None):
        """x [B,1,S,S]: what the sampler returned (in [-1,1], before any map) for the batch that for_rows bound.  Keeps, per slice, the
        largest values seen over its real rows (an ensemble records every sample): |M F(C x) - y| / |y| of x and of the last step's
        x_new (SenseRows leaves it on `bound`), the largest |r| / |b| of the batch's conjugate gradients over all steps, and |x|."""
        idx = bound.idx
        m = idx.shape[0]
        self.residual.scatter_reduce_(0, idx, self._residual(x[:m], idx), 'amax')
        self.residual_before.scatter_reduce_(0, idx, self._residual(bound.x_new[:m], idx), 'amax')
        self.cg_residual.scatter_reduce_(0, idx, bound.cg_max[:m], 'amax')
        self.x_norm.scatter_reduce_(0, idx, _norms(x[:m]), 'amax')

    def reconstruction(self):
        """lambda (I + lambda N)^-1 A^H y [n,S,S] in [-1,1] terms: the step itself, clean, from x_new = 0."""
        from . import ops
        out = torch.empty_like(self.ahy)
        zeros = torch.zeros_like(self.ahy[:1])
        for lo, hi in _chunks(self.n, int(self.maps.shape[0]) * int(self.ahy[0].numel())):
            ops.sense_constrain(zeros.expand(hi - lo, -1, -1).contiguous(), self.ahy[lo:hi], self.mask[lo:hi], self.maps, self.options['lam'],
                                self.options['iters'], None, 0, None, None, clean=True, out=out[lo:hi])
        return out

    def finish(self):
        """The report with the residuals put in (None for a slice that was not measured)."""
        r, flags = self.report, self.report['measured_per_slice']
        for name, v in (('residual', self.residual), ('residual_before', self.residual_before), ('cg_residual', self.cg_residual)):
            v = v.cpu().tolist()
            r[f'{name}_per_slice'] = [a if f else None for a, f in zip(v, flags)]
            r[f'max_{name}'] = max([a for a, f in zip(v, flags) if f], default=None)
        r['y_norm_per_slice'] = self.y_norm.cpu().tolist()       # |y| and the largest |x|: what the residual's rounding scales with
        r['x_norm_per_slice'] = self.x_norm.cpu().tolist()
        if self.options['noise'] > 0:                             # |sigma (n_re + i n_im)| / |y| in expectation: what no x can go below
            count = self.mask.flatten(1).sum(1, dtype=torch.float64) * int(self.maps.shape[0])
            floor = (self.options['noise'] * torch.sqrt(2 * count) / self.y_norm.double().clamp_min(1e-30)).cpu().tolist()
            r['noise_floor_per_slice'] = [a if f else None for a, f in zip(floor, flags)]
        return r


def measure(region, s0, s1, size, options, seed, device):
    """known_region.KnownRegion (K on the prediction's grid: --norm applied, its known mask = coverage AND finite AND not dropped AND
    slab) -> SenseMeasurement for the slab s0..s1 on the S x S sampler grid."""
    from . import known_region as KR
    from . import ops
    S = int(size)
    k, vmask = KR.sampler_inputs(region, s0, s1, S, device)                      # [n,1,S,S] each, resized like the conditions
    measured = vmask.flatten(1).min(1).values != 0                               # every pixel of the slice known
    M = build_mask(S, options['pattern'], options['accel'], options['center'], options['axis'], seed, options['mask_file'])
    mask = (torch.from_numpy(M).to(device)[None] * measured.to(torch.uint8)[:, None, None]).contiguous()
    C = coil_maps(S, options['coils']) if options['maps'] is None else load_maps(options['maps'], S)
    maps = torch.from_numpy(C).to(device)
    n, Nc = int(k.shape[0]), int(maps.shape[0])
    y = torch.empty(n, Nc, S, S, device=device, dtype=torch.complex64)
    ahy = torch.empty(n, S, S, device=device, dtype=torch.float32)
    for lo, hi in _chunks(n, Nc * S * S):
        ops.sense_measure(k[lo:hi, 0].contiguous(), maps, mask[lo:hi], out=y[lo:hi])
        if options['noise'] > 0:
            sl = torch.arange(s0 + lo, s0 + hi, dtype=torch.int64).repeat_interleave(Nc)
            keys = torch.stack([sl, torch.arange(Nc, dtype=torch.int64).repeat(hi - lo)], 1)
            eta = ops.randn_keyed(keys.to(device), 2 * S * S, seed, 0, ops.KIND_SENSE_MEAS)
            eta = torch.view_as_complex(eta.view(hi - lo, Nc, S, S, 2))
            y[lo:hi] += torch.where(mask[lo:hi, None] != 0, options['noise'] * eta, torch.zeros((), device=device, dtype=eta.dtype))
        ops.sense_adjoint(y[lo:hi], maps, out=ahy[lo:hi])
    flags = [bool(v) for v in measured.cpu().tolist()]
    report = dict(pattern=options['pattern'], accel=options['accel'], center=options['center'], axis=options['axis'],
                  mask_file=options['mask_file'], coils=Nc, maps='analytic' if options['maps'] is None else options['maps'],
                  **{'lambda': options['lam']}, iters=options['iters'], noise=options['noise'], image_size=S, slab=[int(s0), int(s1)],
                  sampling_fraction=float(M.mean()), measured_slices=sum(flags), unmeasured_slices=len(flags) - sum(flags),
                  measured_per_slice=flags, drop_slices=region.report['drop_slices'], resample=region.resample,
                  resampled=region.report['resampled'])
    return SenseMeasurement(y, ahy, mask, maps, report, region.resample, options)


def suffix(measurement):
    """What a [done] line gains (nothing without --known_sense)."""
    if measurement is None:
        return ''
    r = measurement.report
    return f" | sense={r['pattern']} x{r['accel']} {r['coils']} coils"
