"""Sample a target that was acquired as accelerated thick slices (--known_multislice; csrc/slab_kspace.hip: mud_slab_kspace_constrain;
DESIGN.md section 5.28).

--known_thick keeps the slab averages of a 2D multi-slice scan and takes every in-plane coefficient of them as measured; --known_kspace
keeps measured coefficients and takes the slices as thin.  The protocol a clinical scanner runs is both at once: thick slices (5 mm,
perhaps with a gap), accelerated in-plane.  With --known_multislice PATTERN --multislice_thick L the thin slices of --known_volume K are
measured retrospectively under the composite model and the sampler keeps what that measures:

    K --known_region's road--> the prediction's grid --norm, resize--> k [n,S,S] --ops.slab_average--> sum_l w_l k_{z_j + l}
      --ops.fft2--> y_j = M_eff * F(.) --> sampler (every step)

The slabs are thick.layout's (--multislice_thick L, --multislice_gap G, --multislice_offset O, of the *volume*), the weights
thick.profile_weights' (--multislice_profile), the mask kspace.build_mask's, symmetrised, one per volume (--multislice_accel,
--multislice_center, --multislice_axis, --multislice_mask_file).  For one slab the operator is A = M F (w^T (x) I) and A A^H =
(sum w^2) M, so the constraint is still an exact projection in closed form: after the reverse step executed with t = i the measured
coefficients of the slab average of x are replaced by those of q_sample(k, i), after the last by y itself; the unmeasured coefficients of
the average and everything orthogonal to the profile are left as the model made them (constraints.SlabKSpaceRows, kind
ops.KIND_MULTISLICE; the draw and --known_resample: mudiff_hip.constraints, section 5.24a).

A slab is measured under thick.measure's rule: complete, inside the sampled range, K known on every pixel of every one of its slices,
none named by --known_drop_slices.  --known_mask, --known_kspace and --known_thick are refused.  The batching keeps a measured slab in
one batch (thick.SlabbedMeasurement), and the written bytes do not depend on --batch_size.

There is no final paste.  multislice_<t>.json lists, per slab, |M_eff (F(sum_l w_l x_l) - y)| / |y| of the sampler's result before it
is mapped to [0,1].  It does not survive clipping, --resize_back, the median or the quantile maps.  --multislice_baseline also writes
multislice_baseline_<t>.nii.gz, what one would have without the model: the zero-filled Re F^H y_j, interpolated linearly along z.

Scope: the single-coil, real-image, retrospective model with non-overlapping profiles.  A NIfTI that is itself thick, overlapping or
fractional profiles, multi-coil complex data, a mask file per slab and the uncaptured sampler path are out of scope.  Whether this helps
a trained model is unmeasured and is not claimed.
"""
from __future__ import annotations

import numpy as np
import torch

from . import kspace as KS
from . import thick as TH
from .constraints import SlabKSpaceRows, need_keyed_seed, need_known_volume

PATTERNS = KS.PATTERNS
_DEPENDENT = ('thick', 'gap', 'offset', 'profile', 'accel', 'center', 'axis', 'mask_file')


def add_flags(p):
    p = p.later() if hasattr(p, 'later') else p          # volume.VolumeParser: the lists of the parsers before this one are pinned
    p.add_argument('--known_multislice', type=str, default=None, choices=list(PATTERNS),
                   help='with --known_volume K: K was acquired as thick slices that are undersampled in k-space.  Every --multislice_thick '
                        'consecutive thin slices of K are averaged under the slice profile, the average is measured with this sampling '
                        'pattern, and the measured coefficients are re-imposed after every reverse step (mudiff_hip.multislice, DESIGN.md '
                        'section 5.28); --known_drop_slices then means `this thick slice was not acquired`')
    p.add_argument('--multislice_thick', type=int, default=None, metavar='L', help=f'thin slices per thick slice, 1..{TH.MAX_L} (required)')
    p.add_argument('--multislice_gap', type=int, default=None, metavar='G', help='unmeasured thin slices between slabs (default 0)')
    p.add_argument('--multislice_offset', type=int, default=None, metavar='O',
                   help='the thin slice of the volume where the first slab starts (default 0)')
    p.add_argument('--multislice_profile', type=str, default=None, choices=list(TH.PROFILES),
                   help='the slice profile, box (equal weights, the default) or gauss (FWHM = L slices)')
    p.add_argument('--multislice_accel', type=int, default=None, metavar='R',
                   help=f'for equispaced / random: the in-plane acceleration, an integer >= 1 (default {KS.DEFAULT_ACCEL})')
    p.add_argument('--multislice_center', type=float, default=None, metavar='F',
                   help=f'the fraction of fully sampled central lines; for lowres the central round(F * S)^2 square (default {KS.DEFAULT_CENTER})')
    p.add_argument('--multislice_axis', type=int, default=None, choices=[0, 1], help=f'the phase-encode axis of the slice (default {KS.DEFAULT_AXIS})')
    p.add_argument('--multislice_mask_file', type=str, default=None, metavar='M.npy',
                   help='with --known_multislice file: uint8 [S, S], non-zero = measured, centred (DC at [S/2, S/2]); one mask for every slab')
    p.add_argument('--multislice_baseline', action='store_true',
                   help='also write multislice_baseline_<t>.nii.gz: the zero-filled Re F^H y of every thick slice, interpolated linearly along '
                        'z (what one would have without the model; scored too under --gt_volume)')


def options_from(args):
    """A namespace's --known_multislice / --multislice_* flags (any may be missing) -> None without --known_multislice, else dict(pattern,
    L, gap, offset, profile, accel, center, axis, mask_file, baseline).  ValueError, naming the flag, for a dependent flag without
    --known_multislice, a missing --multislice_thick, --known_multislice without --known_volume (a cohort's namespace excepted: its K is
    the manifest's `known` column) or with --known_mask, --known_kspace or --known_thick, an --image_size the transform does not take, a
    bad value and a seed outside [0, 2^64)."""
    pattern = getattr(args, 'known_multislice', None)
    v = {f: getattr(args, 'multislice_' + f, None) for f in _DEPENDENT}
    baseline = bool(getattr(args, 'multislice_baseline', False))
    if pattern is None:
        for f in _DEPENDENT:
            if v[f] is not None:
                raise ValueError(f'--multislice_{f} needs --known_multislice')
        if baseline:
            raise ValueError('--multislice_baseline needs --known_multislice')
        return None
    if pattern not in PATTERNS:
        raise ValueError(f'--known_multislice must be one of {PATTERNS}, got {pattern!r}')
    need_known_volume(args, '--known_multislice')
    if getattr(args, 'known_mask', None) is not None:
        raise ValueError('--known_multislice cannot be combined with --known_mask (a thick slice is measured in k-space; use '
                         '--known_drop_slices for thick slices that were not acquired)')
    for other in ('known_kspace', 'known_thick'):
        if getattr(args, other, None) is not None:
            raise ValueError(f'--known_multislice cannot be combined with --{other} (it is both at once: its own --multislice_* flags say '
                             'how thick and how accelerated)')
    L = v['thick']
    if L is None:
        raise ValueError('--known_multislice needs --multislice_thick L (thin slices per thick slice)')
    TH.thickness('--multislice_thick', L)                 # (a bad L is named before a bad --image_size)
    from .ops import kspace_size_ok
    size = getattr(args, 'image_size', None)
    if size is not None and not kspace_size_ok(size):
        raise ValueError(f'--known_multislice needs an --image_size that is a power of two in [16, 512], got {size}')
    slab = TH.slab_options('--multislice_thick', '--multislice_', L, v['gap'], v['offset'], v['profile'])
    sampling = KS.pattern_options('--known_multislice', '--multislice_', pattern, v['accel'], v['center'], v['axis'], v['mask_file'])
    need_keyed_seed(args, '--known_multislice', 'its draws and its mask are keyed')
    return dict(pattern=pattern, **slab, **sampling, baseline=baseline)


# ---------------------------------------------------------------------------------------------------
# the measurement of one prediction
# ---------------------------------------------------------------------------------------------------
class MultisliceMeasurement(TH.SlabbedMeasurement):
    """What the samplers take for one prediction of n thin slices: `y` complex64 [G,S,S] on the device, the measured coefficients of the
    measured slabs' averages, and `mask` uint8 [1,S,S], M_eff; the slabs (`starts`, `group_of`, `weights`, `gains`, `L`) and the batching
    as thick.ThickMeasurement's; `report`: multislice_<t>.json; `resample`: --known_resample."""

    def __init__(self, y, mask, starts, n, weights, report, resample, options):
        super().__init__(y, starts, n, weights, report, resample, options)
        self.mask = mask

    tag, baseline_through_plane = 'multislice', True
    done_suffix = lambda self: suffix(self)      # noqa: E731
    baseline = lambda self: ('multislice_baseline', self.zero_filled_interpolated()) if self.options['baseline'] else None      # noqa: E731

    def for_rows(self, slices, samples=None, m=None):
        """group_rows' batch -> constraints.SlabKSpaceRows = (the tuple mud_slab_kspace_constrain's wrapper takes, the measured slab of
        each group)."""
        members, gids = self.group_rows(slices, samples, m)
        idx = torch.as_tensor(gids, dtype=torch.int64, device=self.y.device)
        return SlabKSpaceRows((self.y.index_select(0, idx), self.mask, members, self.weights, self.gains), idx)

    def difference(self, operands, ax):
        """M_eff (F(A x) - y) of the batch's groups: `record` keeps |M_eff (F(sum_l w_l x_l) - y)| / |y|."""
        from . import ops
        F = ops.fft2(ax)
        return torch.where(operands[1] != 0, F - operands[0], torch.zeros((), device=F.device, dtype=F.dtype))

    def zero_filled_interpolated(self):
        """[n,S,S] in [-1,1] terms: Re F^H y_j per measured slab, interpolated along z as thick.interpolate_slabs does."""
        from . import ops
        S = self.y.shape[-1]
        z = ops.fft2(self.y, inverse=True).real.contiguous() if self.y.shape[0] else torch.zeros(0, S, S, device=self.y.device)
        return TH.interpolate_slabs(z, self.starts, self.L, self.n)


def measure(region, s0, s1, size, options, seed, device):
    """known_region.KnownRegion (K on the prediction's grid: --norm applied, its known mask = coverage AND finite AND not dropped AND
    sampled range) -> MultisliceMeasurement for the thin slices s0..s1 on the S x S sampler grid."""
    from . import ops
    S, L = int(size), options['L']
    k, starts, slabs, w32, head, tail = TH.select_slabs(region, int(s0), int(s1), S, options, device)
    M = KS.build_mask(S, options['pattern'], options['accel'], options['center'], options['axis'], seed, options['mask_file'])
    M_eff = KS.symmetrise(M)
    mask = torch.from_numpy(M_eff).to(device)[None].contiguous()
    if starts:
        members = np.asarray([list(range(s, s + L)) for s in starts], np.int32)
        F = ops.fft2(ops.slab_average(k[:, 0].contiguous(), members, w32))
        y = torch.where(mask != 0, F, torch.zeros((), device=device, dtype=F.dtype)).contiguous()
    else:
        y = torch.zeros(0, S, S, device=device, dtype=torch.complex64)
    report = dict(pattern=options['pattern'], accel=options['accel'], center=options['center'], axis=options['axis'],
                  mask_file=options['mask_file'], **head, given_fraction=float(M.mean()), effective_fraction=float(M_eff.mean()), slabs=slabs,
                  **tail)
    return MultisliceMeasurement(y, mask, starts, int(k.shape[0]), w32, report, region.resample, options)


def suffix(measurement):
    """What a [done] line gains (nothing without --known_multislice)."""
    if measurement is None:
        return ''
    r = measurement.report
    return f" | multislice={r['L']}+{r['gap']} {r['profile']} {r['pattern']} x{r['accel']} ({r['measured_slabs']}/{len(r['slabs'])} slabs)"
